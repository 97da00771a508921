"""GPU tests of the GAN-objective kernels (bg_gan_d_loss, bg_gan_g_loss, bg_gp_seed_target_f32) against the numpy reference of
tests/objective_reference.py.

Bounds.  Hinge and Wasserstein seeds, and the seed kernel at t = 0 and t = 1, are compared bit for bit (with the float32 formula,
with coef * g, with the kernels that exist).  Nonsaturating seeds: |error| <= 16 * 2^-24 * |float64 value| + 2^-126 -- a sigmoid is
an exponential, an addition and a division, each within an ulp or two, the product with w one rounding more; below the smallest
normal float32 (exp(-100) = 3.7e-44) the format itself keeps no relative precision, hence the absolute term.  The seed kernel at
t = 0.5: three roundings, the same relative 16 * 2^-24.  A metric slot, a sum of B float32 terms in a fixed order with a handful of
operations per term and after the sum: (B + 16) * 2^-24 * sum |terms|."""
import ctypes as C

import numpy as np
import pytest
import torch

from blurred_gan_amd import _lib, ops
from helpers import Guarded
import objective_reference as OR

pytestmark = pytest.mark.gpu

F32 = np.float32
LOSSES = ["wasserstein", "hinge", "nonsaturating"]
SPECIAL = np.array([-2, -1, np.nextafter(F32(-1), F32(0)), 0, np.nextafter(F32(1), F32(0)), 1, 2, 30, -30, 100, -100], F32)
PAR = dict(inv_gbs=1 / 7, gp_coef=10.0, e_drift=1e-4, vec_scale=5.0)       # w = 5 / 7: the product is not exact in float32


def scores(B, seed):
    """fs, rs, norms [B] float32: normal scores of spread 1.5 with the special values placed (cyclically shifted between the two)."""
    rng = np.random.default_rng(seed)
    fs, rs = (rng.normal(size=B) * 1.5).astype(F32), (rng.normal(size=B) * 1.5).astype(F32)
    k = min(B, SPECIAL.size)
    at = rng.permutation(B)[:k]
    fs[at], rs[at] = SPECIAL[:k], np.roll(SPECIAL, 3)[:k]
    return fs, rs, np.abs(rng.normal(size=B) + 1).astype(F32)


def put(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def metric_close(got, ref, B, what):
    bound = (B + 16) * 2.0 ** -24 * ref["mag"]
    err = np.abs(got.astype(np.float64) - ref["met"])
    print(f"[{what}] B={B} metric errors {err} bounds {bound}")
    assert np.all(err <= bound), (what, err, bound)


@pytest.mark.parametrize("e_drift", [1e-4, 0.0])
@pytest.mark.parametrize("t", [1.0, 0.0, 0.5])
@pytest.mark.parametrize("B", [1, 5, 255, 256, 257, 515])
@pytest.mark.parametrize("loss", LOSSES)
def test_d_loss(loss, B, t, e_drift):
    fs, rs, norms = scores(B, B)
    par = dict(PAR, e_drift=e_drift)
    for with_norm in (True, False):
        dfs, drs, met = Guarded(B), Guarded(B), Guarded(6)
        ops.objective.d_loss(put(fs), put(rs), put(norms) if with_norm else None, OR.LOSS[loss], par["inv_gbs"], par["gp_coef"], t, e_drift,
                             par["vec_scale"], dfs.view, drs.view, met.view)
        assert dfs.guards_intact() and drs.guards_intact() and met.guards_intact()
        ref = OR.np_d_loss(fs, rs, norms if with_norm else None, loss, F32(par["inv_gbs"]), F32(par["gp_coef"]), F32(t), F32(e_drift), F32(par["vec_scale"]))
        f32 = OR.np_d_loss(fs, rs, norms if with_norm else None, loss, par["inv_gbs"], par["gp_coef"], t, e_drift, par["vec_scale"], dtype=F32)
        for name, got in (("dfs", dfs.get()), ("drs", drs.get())):
            assert np.isfinite(got).all(), name
            if loss == "nonsaturating":
                err, bound = np.abs(got.astype(np.float64) - ref[name]), OR.FLOOR * np.abs(ref[name]) + OR.TINY
                print(f"[{loss} {name}] B={B} max error / bound {float((err / bound).max()):.3f}")
                assert np.all(err <= bound), (name, float((err / bound).max()))
            else:
                assert np.array_equal(bits(got), bits(f32[name])), name
        metric_close(met.get(), ref, B, f"d_loss {loss} t={t} norm={with_norm}")
        if not with_norm:
            assert met.get()[3] == 0 and met.get()[5] == 0


@pytest.mark.parametrize("B", [1, 5, 255, 256, 257, 515])
def test_wasserstein_at_target_one_is_the_existing_kernel_bit_for_bit(B):
    fs, rs, norms = scores(B, B + 1000)
    for n in (put(norms), None):
        out = [(Guarded(B), Guarded(B), Guarded(6)) for _ in range(2)]
        ops.wgangp_d_loss(put(fs), put(rs), n, PAR["inv_gbs"], PAR["gp_coef"], PAR["e_drift"], PAR["vec_scale"], *(g.view for g in out[0]))
        ops.objective.d_loss(put(fs), put(rs), n, OR.LOSS["wasserstein"], PAR["inv_gbs"], PAR["gp_coef"], 1.0, PAR["e_drift"], PAR["vec_scale"],
                             *(g.view for g in out[1]))
        for a, b in zip(*out):
            assert np.array_equal(bits(a.get()), bits(b.get())) and b.guards_intact()


@pytest.mark.parametrize("B", [1, 5, 255, 256, 257, 515])
@pytest.mark.parametrize("loss", LOSSES)
def test_g_loss(loss, B):
    s, _, _ = scores(B, B + 7)
    ds, met = Guarded(B), Guarded(2)
    ops.objective.g_loss(put(s), OR.LOSS[loss], PAR["inv_gbs"], ds.view, met.view)
    assert ds.guards_intact() and met.guards_intact()
    ref = OR.np_g_loss(s, loss, F32(PAR["inv_gbs"]))
    got = ds.get()
    assert np.isfinite(got).all()
    if loss == "nonsaturating":
        err, bound = np.abs(got.astype(np.float64) - ref["ds"]), OR.FLOOR * np.abs(ref["ds"]) + OR.TINY
        assert np.all(err <= bound), float((err / bound).max())
    else:
        old_ds, old_met = Guarded(B), Guarded(2)
        ops.wgan_g_loss(put(s), PAR["inv_gbs"], old_ds.view, old_met.view)
        assert np.array_equal(bits(got), bits(old_ds.get())) and np.array_equal(bits(met.get()), bits(old_met.get()))
        assert np.array_equal(bits(got), bits(OR.np_g_loss(s, loss, PAR["inv_gbs"], dtype=F32)["ds"]))
    metric_close(met.get(), ref, B, f"g_loss {loss}")


# ------------------------------------------------------------------ the seed
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset_by_one_float"])
@pytest.mark.parametrize("guard", [False, True], ids=["unguarded", "guarded"])
@pytest.mark.parametrize("t", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("shape", [(3, 5), (2, 12288), (3, 12290)])
def test_gp_seed_target(shape, t, guard, offset):
    B, n_per = shape
    rng = np.random.default_rng(B * n_per)
    g = rng.normal(size=shape).astype(F32)
    g[1] = 0                                             # one sample of zero norm
    norms = np.sqrt((g.astype(np.float64) ** 2).sum(1)).astype(F32)
    assert norms[1] == 0
    coef = 0.7
    src, out = Guarded(B * n_per, init=g, offset=offset), Guarded(B * n_per, offset=offset)
    ops.objective.gp_seed(src.t(B, n_per), put(norms), coef, t, out.t(B, n_per), zero_norm_guard=guard)
    assert out.guards_intact() and src.guards_intact() and src.unchanged()
    got = out.get(B, n_per)
    if t == 0.0:
        assert np.array_equal(bits(got), bits(F32(coef) * g)) and not np.isnan(got).any()
    elif t == 1.0:
        old = Guarded(B * n_per, offset=offset)
        ops.gp_seed(src.t(B, n_per), put(norms), coef, old.t(B, n_per), zero_norm_guard=guard)
        assert np.array_equal(bits(got), bits(old.get(B, n_per)))
    ref = OR.np_gp_seed(g, norms, F32(coef), F32(t), guard)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    assert np.isnan(got[1]).all() == (t > 0 and not guard) and (guard or t == 0) == bool((got[1] == 0).all())
    live = ~np.isnan(ref)
    assert np.all(np.abs(got.astype(np.float64) - ref)[live] <= OR.FLOOR * np.abs(ref)[live])
    # in place, as the step writes the seed over the gradient it came from
    ops.objective.gp_seed(src.t(B, n_per), put(norms), coef, t, src.t(B, n_per), zero_norm_guard=guard)
    assert np.array_equal(bits(src.get(B, n_per)), bits(got)) and src.guards_intact()


# ------------------------------------------------------------------ refusals
def test_refused_calls_return_the_error_code_and_leave_the_outputs_untouched():
    lib = _lib.load()
    B = 5
    fs, rs, norms = (put(a) for a in scores(B, 3))
    init = np.arange(B, dtype=F32)
    dfs, drs, met = Guarded(B, init=init), Guarded(B, init=init), Guarded(6, init=np.arange(6, dtype=F32))
    p = lambda t: C.c_void_p(t.data_ptr())
    d = lambda fs_=p(fs), rs_=p(rs), B_=B, loss=1, t=1.0, dfs_=p(dfs.view), met_=p(met.view): lib.bg_gan_d_loss(
        fs_, rs_, p(norms), B_, loss, 0.2, 10.0, t, 1e-4, 4.0, dfs_, p(drs.view), met_, None)
    assert d(fs_=None) == -6 and d(rs_=None) == -6 and d(dfs_=None) == -6 and d(met_=None) == -6
    assert d(B_=0) == -1 and d(B_=-3) == -1
    assert d(loss=3) == -3 and d(loss=-1) == -3 and d(t=-0.5) == -3
    assert b"bg_gan_d_loss" in lib.bg_last_error()
    g = lambda s_=p(fs), B_=B, loss=2, ds_=p(dfs.view), met_=p(met.view): lib.bg_gan_g_loss(s_, B_, loss, 0.2, ds_, met_, None)
    assert g(s_=None) == -6 and g(ds_=None) == -6 and g(met_=None) == -6 and g(B_=0) == -1 and g(loss=7) == -3
    grad = put(np.ones((B, 4), F32))
    out = Guarded(B * 4, init=np.arange(B * 4, dtype=F32))
    s = lambda g_=p(grad), n_=p(norms), t=0.5, out_=p(out.view), B_=B, n_per=4: lib.bg_gp_seed_target_f32(g_, n_, 0.7, t, 0, out_, B_, n_per, None)
    assert s(g_=None) == -6 and s(n_=None) == -6 and s(out_=None) == -6
    assert s(B_=0) == -1 and s(n_per=0) == -1 and s(t=-1.0) == -3
    torch.cuda.synchronize()
    for buf in (dfs, drs, met, out):
        assert buf.unchanged() and buf.guards_intact()
