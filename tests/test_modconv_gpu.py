"""GPU tests of the StyleModulation kernels (csrc/modconv.hip) against tests/modconv_reference.py: the scale bit for bit against
numpy float32 arithmetic, the pixel sums exactly on integer data and inside their rounding bound on normal data, Q, the
demodulation and the two gradients against float64, 16-byte aligned and one float off.

Shapes: C in {3, 4, 32, 132, 260, 512, 1028} (single floats, one float4, eight, 33 in a wave, two per lane twice, a row in chunks;
one float off: 132 by fours per lane, 260 and up in scalar chunks), P in {1, 3, 16, 67} (at 1 and 3 a wave's rows straddle samples),
B in {1, 5}; one dot at P = 4096, C = 32, B = 8 takes the slab route."""
import itertools

import numpy as np
import pytest
import torch

from blurred_gan_amd import ops
from helpers import Guarded
import modconv_reference as MC

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
CS, PS, BS = (3, 4, 32, 132, 260, 512, 1028), (1, 3, 16, 67), (1, 5)
SHAPES = list(itertools.product(CS, PS, BS))
ids = lambda s: "c%d_p%d_b%d" % s


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _ints(rng, lo, hi, *shape):
    return rng.integers(lo, hi + 1, size=shape).astype(np.float32)


def test_the_shapes_reach_every_route():
    seen = set()
    for C in CS:
        for aligned in (True, False):
            r = ops.noise.route(C, aligned)         # csrc/rowwise.h's routes: the ones bg_mod_scale_f32 takes
            seen.add((r["vec"], r["regs"], r["chunks"] > 1))
    assert seen >= {(1, 1, False), (4, 1, False), (4, 2, False), (1, 4, False), (1, 1, True), (4, 1, True)}, seen
    # one slab wherever the sample's pixels are at most 16 visits of the workgroup (256 / lanes pixels a visit); of the grid's
    # shapes only the widest rows at P = 67 are cut, the large case is the slab route proper
    plans = {(C, P, B): ops.modconv.dot_plan(B, P, C) for C, P, B in SHAPES}
    assert all(p["slabs"] == 1 for (C, P, B), p in plans.items() if P <= 16 * (256 // p["lanes"]))
    assert all(p["slabs"] == 1 for (C, P, B), p in plans.items() if P <= 16) and plans[(32, 67, 5)]["slabs"] == 1
    p = ops.modconv.dot_plan(8, 4096, 32)
    u = ops.modconv.dot_plan(8, 4096, 32, aligned=False)
    assert p["slabs"] > 1 and p["vec"] == 4 and u["slabs"] > 1 and u["vec"] == 1
    assert ops.modconv.dot_workspace_bytes(8, 4096, 32) == 4 * 8 * 32 * max(p["slabs"], u["slabs"])         # room for either route


# ------------------------------------------------------------------ scale
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_scale_is_numpy_float32_bit_for_bit(shape):
    C, P, B = shape
    rng = np.random.default_rng(C * 1000 + P * 10 + B)
    x, v, bias = (rng.normal(size=s).astype(np.float32) for s in ((B, P, C), (B, C), (C,)))
    for off, with_bias, alpha, inplace in itertools.product((0, 1), (False, True), (1.0, 0.2), (False, True)):
        gx, gv, gb = Guarded(x.size, x, offset=off), Guarded(v.size, v, offset=off), Guarded(C, bias, offset=off)
        go = gx if inplace else Guarded(x.size, offset=off)
        ops.modconv.scale(gx.view, gv.view, go.view, B, P, C, bias=gb.view if with_bias else None, lrelu_alpha=alpha)
        want = MC.np_scale(x, v, bias if with_bias else None, alpha)
        what = (shape, off, with_bias, alpha, inplace)
        assert np.array_equal(_bits(go.get(B, P, C)), _bits(want)), what
        assert go.guards_intact() and gv.unchanged() and gb.unchanged() and (inplace or gx.unchanged()), what


# ------------------------------------------------------------------ dot
def _dot(a, b, B, P, C, off, old=None, beta=0.0, scale=1.0):
    ga, gb = Guarded(a.size, a, offset=off), Guarded(b.size, b, offset=off)
    go = Guarded(B * C, old, offset=off)
    nb = ops.modconv.dot_workspace_bytes(B, P, C)
    ws = torch.empty(nb // 4 + 4, device="cuda") if nb else None
    ops.modconv.dot(ga.view, gb.view, go.view, B, P, C, ws, beta=beta, scale=scale)
    assert go.guards_intact() and ga.unchanged() and gb.unchanged()
    return go.get(B, C)


@pytest.mark.parametrize("shape", SHAPES + [(32, 4096, 8)], ids=ids)
def test_dot_exact_on_integers_and_inside_the_bound_on_normal_data(shape):
    C, P, B = shape
    rng = np.random.default_rng(C * 1000 + P * 10 + B + 1)
    assert 64 * P * 2 + 64 < 1 << 24
    for off in (0, 1):
        a, b, old = _ints(rng, -8, 8, B, P, C), _ints(rng, -8, 8, B, P, C), _ints(rng, -8, 8, B, C)
        ref, _ = MC.np_dot(a, b)
        assert np.array_equal(_dot(a, b, B, P, C, off), ref.astype(np.float32)), (shape, off)
        ref, _ = MC.np_dot(a, b, old, beta=0.5, scale=2.0)          # beta / scale honoured (powers of two: still exact)
        assert np.array_equal(_dot(a, b, B, P, C, off, old, 0.5, 2.0), ref.astype(np.float32)), (shape, off)
        x, y = rng.normal(size=(B, P, C)).astype(np.float32), rng.normal(size=(B, P, C)).astype(np.float32)
        got = _dot(x, y, B, P, C, off)
        ref, mag = MC.np_dot(x, y)
        err = np.abs(got.astype(np.float64) - ref)
        print(f"{shape} off {off}: max err / bound {float((err / ((P + 8) * U * mag + 1e-300)).max()):.3f}")
        assert (err <= (P + 8) * U * mag).all(), (shape, off)
        assert np.array_equal(_bits(_dot(x, y, B, P, C, off)), _bits(got)), (shape, off)         # two runs: the same bits


# ------------------------------------------------------------------ Q and its gradient
WSQ = [(k, I, O, tr) for k in (1, 3, 5) for (I, O) in ((3, 5), (32, 16), (70, 33)) for tr in (False, True)]


@pytest.mark.parametrize("k,I,O,tr", WSQ)
def test_wsq_both_layouts(k, I, O, tr):
    rng = np.random.default_rng(k * 100 + I + O + tr)
    shape = (k, k, O, I) if tr else (k, k, I, O)
    for off in (0, 1):
        w = _ints(rng, -8, 8, *shape)
        gw, gq = Guarded(w.size, w, offset=off), Guarded(I * O, offset=off)
        ops.modconv.wsq(gw.view, gq.view, k * k, I, O, transposed=tr)
        assert np.array_equal(gq.get(I, O), MC.np_wsq(w, tr).astype(np.float32)) and gq.guards_intact() and gw.unchanged()
        w = rng.normal(size=shape).astype(np.float32)
        gw, gq = Guarded(w.size, w, offset=off), Guarded(I * O, offset=off)
        ops.modconv.wsq(gw.view, gq.view, k * k, I, O, transposed=tr)
        ref = MC.np_wsq(w, tr)
        assert (np.abs(gq.get(I, O).astype(np.float64) - ref) <= (k * k + 8) * U * ref).all()


@pytest.mark.parametrize("k,I,O,tr", WSQ)
def test_wsq_grad_both_layouts(k, I, O, tr):
    rng = np.random.default_rng(k * 100 + I + O + tr + 7)
    shape = (k, k, O, I) if tr else (k, k, I, O)
    for off, exact in itertools.product((0, 1), (True, False)):
        draw = (lambda *s: _ints(rng, -8, 8, *s)) if exact else (lambda *s: rng.normal(size=s).astype(np.float32))
        w, dQ, dw = draw(*shape), draw(I, O), draw(*shape)
        scale = 0.25 if exact else 0.3
        gw, gq, gd = Guarded(w.size, w, offset=off), Guarded(I * O, dQ, offset=off), Guarded(w.size, dw, offset=off)
        ops.modconv.wsq_grad(gw.view, gq.view, gd.view, k * k, I, O, transposed=tr, scale=scale)
        ref = MC.np_wsq_grad(w, dQ, dw, tr, np.float64(np.float32(scale)))
        got = gd.get(*shape)
        assert gd.guards_intact() and gw.unchanged() and gq.unchanged()
        if exact:
            assert np.array_equal(got, ref.astype(np.float32))
        else:
            mag = np.abs(dw.astype(np.float64)) + np.abs(ref - dw)
            assert (np.abs(got - ref) <= (2 + 8) * U * mag).all()


# ------------------------------------------------------------------ demodulation
DEMOD = list(itertools.product((3, 32, 512), (3, 16, 512), (1, 5)))


@pytest.mark.parametrize("I,O,B", DEMOD)
def test_demod_against_float64(I, O, B):
    rng = np.random.default_rng(I + O + B)
    for off in (0, 1):
        s = rng.normal(size=(B, I)).astype(np.float32)
        Q = (rng.normal(size=(I, O)) ** 2 * 9).astype(np.float32)
        gs, gq, gd = Guarded(s.size, s, offset=off), Guarded(Q.size, Q, offset=off), Guarded(B * O, offset=off)
        ops.modconv.demod(gs.view, gq.view, gd.view, B, I, O, eps=1e-8)
        ref = MC.np_demod(s, Q, np.float64(np.float32(1e-8)))
        rel = np.abs(gd.get(B, O).astype(np.float64) - ref) / ref
        print(f"I={I} O={O} B={B} off {off}: max rel err / bound {float(rel.max() / ((I / 2 + 8) * U)):.3f}")
        assert (rel <= (I / 2 + 8) * U).all() and gd.guards_intact() and gs.unchanged() and gq.unchanged()
    # exact where it can be: one channel, s and Q powers of two with an even exponent sum, eps far below half an ulp
    s, Q = np.array([[4.0]], np.float32), np.array([[0.25, 1.0, 4.0]], np.float32)
    d = torch.empty(1, 3, device="cuda")
    ops.modconv.demod(torch.from_numpy(s).cuda(), torch.from_numpy(Q).cuda(), d, 1, 1, 3, eps=1e-8)
    assert np.array_equal(d.cpu().numpy(), np.array([[0.5, 0.25, 0.125]], np.float32))


@pytest.mark.parametrize("I,O,B", DEMOD)
def test_demod_bwd_against_float64(I, O, B):
    rng = np.random.default_rng(I + O + B + 3)
    for off, exact in itertools.product((0, 1), (True, False)):
        if exact:       # d powers of two, the rest small integers: every product and every partial sum is an integer multiple of 2^-10
            d = (2.0 ** rng.integers(-3, 1, size=(B, O))).astype(np.float32)
            dd, s, Q, ds = _ints(rng, -4, 4, B, O), _ints(rng, -4, 4, B, I), _ints(rng, 0, 4, I, O), _ints(rng, -8, 8, B, I)
        else:
            d = (0.1 + rng.uniform(size=(B, O))).astype(np.float32)
            dd, s, ds = (rng.normal(size=sh).astype(np.float32) for sh in ((B, O), (B, I), (B, I)))
            Q = (rng.normal(size=(I, O)) ** 2).astype(np.float32)
        g = {n: Guarded(a.size, a, offset=off) for n, a in dict(d=d, dd=dd, s=s, Q=Q, ds=ds).items()}
        gdq = Guarded(B * O, offset=off)
        ops.modconv.demod_bwd(g["d"].view, g["dd"].view, g["s"].view, g["Q"].view, gdq.view, g["ds"].view, B, I, O)
        dq, ds_ref, mag = MC.np_demod_bwd(d, dd, s, Q, ds)
        got_dq, got_ds = gdq.get(B, O), g["ds"].get(B, I)
        assert gdq.guards_intact() and g["ds"].guards_intact() and all(g[n].unchanged() for n in ("d", "dd", "s", "Q"))
        if exact:
            assert np.array_equal(got_dq, dq.astype(np.float32)) and np.array_equal(got_ds, ds_ref.astype(np.float32))
        else:
            assert (np.abs(got_dq - dq) <= 4 * U * np.abs(dq)).all()
            bound = (O + 8) * U * (np.abs(ds.astype(np.float64)) + 2 * np.abs(s.astype(np.float64)) * mag)
            assert (np.abs(got_ds - ds_ref) <= bound).all()


def test_argument_errors_are_statuses():
    x = torch.zeros(16, device="cuda")
    with pytest.raises(ValueError, match="bg_mod_scale_f32"):
        ops.modconv.scale(x[:0], x[:0], x[:0], 0, 1, 1)
    with pytest.raises(ValueError, match="bg_mod_demod_f32"):
        ops.modconv.demod(x[:2], x[:4], x[:2], 1, 2, 2, eps=0.0)
