"""CPU tests of the GAN objectives: the configuration class and its normaliser, the model surface, the demos' flags, the boundary
(symbols, refusals that launch nothing) and the float64 reference of tests/objective_reference.py itself."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import blurred_gan_amd as bg
from blurred_gan_amd import _lib
from blurred_gan_amd.objective import Objective, as_objective
import objective_reference as OR

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_spec = importlib.util.spec_from_file_location("make_engine_trace", os.path.join(HERE, "golden", "make_engine_trace.py"))
maker = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(maker)
NAMES = ("bg_gan_d_loss", "bg_gan_g_loss", "bg_gp_seed_target_f32")


@pytest.fixture(scope="module")
def lib():
    maker.ensure_library(ROOT)
    return _lib.load()


def _gan(cls=None, **kw):
    return maker._gan(bg, cls or bg.BlurredWGANGP, **kw)


# ------------------------------------------------------------------ 1. configuration
def test_defaults_are_the_reference_objective():
    o = Objective()
    assert (o.loss, o.penalty_target, o.penalty_on, o.penalty_interval) == ("wasserstein", 1.0, "interpolates", 1)
    assert o.is_reference and o.has_default_penalty and o.penalty_alpha is None
    assert as_objective(None) == o and as_objective("wasserstein") == o and as_objective(o) is o
    assert as_objective("hinge") == Objective(loss="hinge") and not as_objective("hinge").is_reference
    assert not Objective(penalty_interval=2).is_reference and not Objective(penalty_target=0.0).is_reference
    assert Objective(penalty_on="reals").penalty_alpha == 0.0 and Objective(penalty_on="fakes").penalty_alpha == 1.0
    assert isinstance(Objective(penalty_target=0).penalty_target, float)


@pytest.mark.parametrize("kw", [dict(loss="lsgan"), dict(loss=None), dict(loss=1), dict(penalty_target=-0.1), dict(penalty_target="1"),
                                dict(penalty_target=float("nan")), dict(penalty_target=float("inf")), dict(penalty_target=True),
                                dict(penalty_on="both"), dict(penalty_on=0), dict(penalty_interval=0), dict(penalty_interval=-2),
                                dict(penalty_interval=1.5), dict(penalty_interval=True)])
def test_bad_fields_are_refused(kw):
    with pytest.raises(ValueError):
        Objective(**kw)


def test_bad_objective_arguments_are_refused_before_anything_is_built():
    for bad in (7, "lsgan", ["hinge"]):
        with pytest.raises(ValueError):
            as_objective(bad)

    class Unbuildable:
        def build(self):
            raise AssertionError("built before the objective was checked")
    hp = bg.WGANGP.HyperParameters()
    with pytest.raises(ValueError):
        bg.WGANGP(Unbuildable(), Unbuildable(), hp, bg.TrainingConfig(), objective="lsgan")


def test_penalty_fields_on_a_class_without_penalty_are_refused():
    for kw in (dict(penalty_target=0.0), dict(penalty_on="reals"), dict(penalty_interval=4)):
        for cls in (bg.WGAN, bg.BlurredWGAN):
            with pytest.raises(ValueError, match="no gradient penalty"):
                _gan(cls, blur=cls is bg.BlurredWGAN, objective=Objective("hinge", **kw))
        assert _gan(bg.WGANGP, blur=False, objective=Objective("hinge", **kw)).objective == Objective("hinge", **kw)
    assert _gan(bg.WGAN, blur=False, objective="hinge").objective == Objective("hinge")        # the SN-GAN set-up


def test_config_round_trip():
    a = Objective("nonsaturating", penalty_target=0, penalty_on="reals", penalty_interval=16)
    b = Objective.from_config(a.get_config())
    assert a == b and hash(a) == hash(b) and repr(a) == repr(b)
    assert b.get_config() == {"loss": "nonsaturating", "penalty_target": 0.0, "penalty_on": "reals", "penalty_interval": 16}
    assert a != Objective("nonsaturating") and a != "nonsaturating"


def test_static_config_distinguishes_every_field():
    variants = [Objective(), Objective("hinge"), Objective("nonsaturating"), Objective(penalty_target=0.0), Objective(penalty_target=0.5),
                Objective(penalty_on="reals"), Objective(penalty_on="fakes"), Objective(penalty_interval=2), Objective(penalty_interval=4)]
    keys = [v.static_config() for v in variants]
    assert len(set(keys)) == len(keys) and all(hash(k) is not None for k in keys)
    assert Objective("hinge").static_config() == Objective("hinge").static_config()


def test_penalty_phase():
    o = Objective(penalty_interval=4)
    assert [o.penalty_at(n) for n in range(9)] == [True, False, False, False, True, False, False, False, True]
    assert all(Objective().penalty_at(n) for n in range(5))


# ------------------------------------------------------------------ 2. model surface
def test_objective_argument_on_every_model_class():
    for cls, blur in ((bg.WGAN, False), (bg.WGANGP, False), (bg.BlurredWGANGP, True), (bg.BlurredWGAN, True)):
        assert _gan(cls, blur=blur).objective == Objective()
        assert _gan(cls, blur=blur, objective="nonsaturating").objective == Objective("nonsaturating")
        o = Objective("hinge")
        gan = _gan(cls, blur=blur, objective=o)
        assert gan.objective is o
        with pytest.raises(AttributeError):
            gan.objective = Objective()
    assert "Objective" in bg.__all__ and bg.Objective is bg.objective.Objective


def test_hyperparameters_gain_no_field():
    assert [f for f in vars(bg.WGANGP.HyperParameters())] == ["learning_rate", "d_steps_per_g_step", "batch_size", "global_batch_size", "optimizer",
                                                              "e_drift", "gp_coefficient"]


def test_step_key_and_penalty_decision_follow_the_phase():
    reals = torch.zeros(2, 8, 8, 3)

    def entry(gan, kind):
        for m in (gan.generator, gan.discriminator):
            bg.optimizers.get_optimizer(m).attach(m.store)
        return [k for k in gan._step_key(kind, reals) if isinstance(k, tuple) and k and k[0] == "objective"]

    lazy = _gan(objective=Objective("nonsaturating", penalty_target=0.0, penalty_on="reals", penalty_interval=2))
    seen = []
    for n in range(4):
        lazy.n_batches.assign(n)
        (d,), (g,) = entry(lazy, "d"), entry(lazy, "g")
        seen.append((lazy._penalty_this_step(), d[2], g[2]))
        assert d[1] == lazy.objective.static_config() == g[1]
    assert seen == [(True, True, None), (False, False, None), (True, True, None), (False, False, None)]
    plain, hinge = _gan(), _gan(objective="hinge")
    assert entry(plain, "d") != entry(hinge, "d") and entry(plain, "d") == entry(_gan(objective=Objective()), "d")
    wgan = _gan(bg.WGAN, blur=False, objective="hinge")
    assert not wgan._penalty_this_step() and entry(wgan, "d")[0][2] is False


def test_value_only_losses_follow_the_objective():
    fs, rs = torch.tensor([-2.0, -1.0, 0.5, 3.0]), torch.tensor([2.0, 1.0, -0.5, -3.0])
    gbs = 2                                                                             # maker._gan's global batch
    for loss in ("wasserstein", "hinge", "nonsaturating"):
        gan = _gan(bg.WGAN, blur=False, objective=loss)
        want_d = OR.critic_loss(loss, fs.double(), rs.double()) / gbs
        want_g = OR.generator_loss(loss, fs.double()) / gbs
        assert abs(float(gan.discriminator_loss(None, None, rs, fs)) - float(want_d)) < 1e-6
        assert abs(float(gan.generator_loss(fs)) - float(want_g)) < 1e-6


def test_a_lazy_step_between_two_penalties_launches_no_penalty_pass_and_draws_less():
    """Under the engine-trace recorders: at n_batches = 1 of an interval of 2 the critic step has no lerp, no row_norm, no gp_seed
    and no alpha draw, and its loss launch is not the reference's; the default objective's launch list is the committed trace's."""
    calls = {}
    for n in (0, 1):
        tr = maker.Trace()
        own = []
        with maker.tracing(bg, tr):
            saved = {k: getattr(bg.ops.objective, k) for k in ("d_loss", "g_loss", "gp_seed")}
            try:
                for k in saved:
                    setattr(bg.ops.objective, k, staticmethod(lambda *a, _k=k, **kw: own.append(_k) or (a[4] if _k == "gp_seed" else None)))
                gan = _gan(objective=Objective("nonsaturating", penalty_target=0.0, penalty_on="reals", penalty_interval=2))
                gan.n_batches.assign(n)
                gan.train_on_batch(np.zeros((2, 8, 8, 3), np.float32))
            finally:
                for k, v in saved.items():
                    setattr(bg.ops.objective, k, staticmethod(v))
        calls[n] = ([c.split("(")[0] for c in tr.calls], own, gan._rng_off)
    names0, own0, off0 = calls[0]
    names1, own1, off1 = calls[1]
    assert own0 == ["d_loss", "d_loss", "gp_seed", "g_loss"] and own1 == ["d_loss", "g_loss"]
    assert "row_norm" in names0 and "row_norm" not in names1 and "gp_seed" not in names0 + names1
    assert "wgangp_d_loss" not in names0 + names1 and "wgan_g_loss" not in names0 + names1
    assert names0.count("uniform") == 2 and names1.count("uniform") == 2          # z_d and z_g; alpha is a fill, never a draw
    assert off0 == off1


# ------------------------------------------------------------------ 3. the demos
@pytest.mark.parametrize("demo", ["demo_mnist", "demo_celeba"])
def test_demos_parse_the_four_flags(demo):
    spec = importlib.util.spec_from_file_location(demo, os.path.join(ROOT, demo + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    parser = mod.make_parser()
    a = parser.parse_args([])
    assert Objective(a.loss, a.penalty_target, a.penalty_on, a.penalty_interval) == Objective()
    a = parser.parse_args(["--loss", "nonsaturating", "--penalty-on", "reals", "--penalty-target", "0", "--penalty-interval", "16"])
    assert Objective(a.loss, a.penalty_target, a.penalty_on, a.penalty_interval) == Objective("nonsaturating", 0.0, "reals", 16)
    for bad in (["--loss", "lsgan"], ["--penalty-on", "both"], ["--penalty-interval", "x"]):
        with pytest.raises(SystemExit):
            parser.parse_args(bad)


# ------------------------------------------------------------------ 4. boundary
def test_header_declares_and_the_binding_binds_the_three_entry_points(lib):
    hdr = open(os.path.join(ROOT, "include", "bgan.h")).read()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        decl = re.search(name + r"\s*\(([^;]*)\)\s*;", hdr).group(1)
        assert len([a for a in re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",") if a.strip()]) == len(_lib.SIGNATURES[name][1]), name
    assert re.search(r"BG_LOSS_WASSERSTEIN\s*=\s*0\s*,\s*BG_LOSS_HINGE\s*=\s*1\s*,\s*BG_LOSS_NONSATURATING\s*=\s*2", hdr)
    assert (_lib.LOSS_WASSERSTEIN, _lib.LOSS_HINGE, _lib.LOSS_NONSATURATING) == (0, 1, 2) == tuple(OR.LOSS[k] for k in ("wasserstein", "hinge", "nonsaturating"))
    assert bg.ops.objective.LOSS == OR.LOSS
    assert lib.bg_version() == 5


def test_argument_errors_are_statuses(lib):
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p).value
    d = lambda fs=p, rs=p + 16, dfs=p + 32, drs=p + 48, met=p + 64, B=2, loss=0, t=1.0: lib.bg_gan_d_loss(fs, rs, None, B, loss, 0.5, 10.0, t, 1e-4, 2.0, dfs, drs, met, None)
    assert d(fs=None) == -6 and d(rs=None) == -6 and d(dfs=None) == -6 and d(drs=None) == -6 and d(met=None) == -6
    assert d(B=0) == -1 and d(loss=3) == -3 and d(loss=-1) == -3 and d(t=-1.0) == -3
    assert b"bg_gan_d_loss" in lib.bg_last_error()
    g = lambda s=p, ds=p + 16, met=p + 32, B=2, loss=2: lib.bg_gan_g_loss(s, B, loss, 0.5, ds, met, None)
    assert g(s=None) == -6 and g(ds=None) == -6 and g(met=None) == -6 and g(B=0) == -1 and g(loss=3) == -3
    s = lambda g_=p, n=p + 64, out=p + 128, B=2, n_per=4, t=0.0: lib.bg_gp_seed_target_f32(g_, n, 0.7, t, 0, out, B, n_per, None)
    assert s(g_=None) == -6 and s(n=None) == -6 and s(out=None) == -6 and s(B=0) == -1 and s(n_per=0) == -1 and s(t=-0.5) == -3
    assert b"bg_gp_seed_target_f32" in lib.bg_last_error()
    assert not any(buf)


def test_cpu_tensors_are_rejected(lib):
    x = torch.zeros(4)
    with pytest.raises(bg.ops.BgDeviceError):
        bg.ops.objective.g_loss(x, 2, 0.5, torch.empty(4), torch.empty(2))
    with pytest.raises(ValueError):
        bg.gradient_penalty(None, None, None, target=-1.0)


# ------------------------------------------------------------------ 5. the reference itself
def test_reference_softplus_and_sigmoid_are_safe_and_consistent():
    x = np.array([-800.0, -100.0, -30.0, -1.0, 0.0, 1.0, 30.0, 100.0, 800.0])
    with np.errstate(over="raise", invalid="raise", divide="raise"):       # exp(-800) underflows to 0, which is the right value
        sp, sg = OR.softplus(x), OR.sigmoid(x)
    assert np.isfinite(sp).all() and np.isfinite(sg).all() and sp[0] == 0 and sp[-1] == 800 and sg[0] == 0 and sg[-1] == 1
    np.testing.assert_allclose(sg + OR.sigmoid(-x), 1.0, rtol=0, atol=1e-15)
    np.testing.assert_allclose(OR.softplus(x) - OR.softplus(-x), x, rtol=1e-13, atol=1e-13)
    mid = x[2:-2]
    np.testing.assert_allclose(sp[2:-2], np.log1p(np.exp(mid)), rtol=1e-12)


@pytest.mark.parametrize("loss", ["wasserstein", "hinge", "nonsaturating"])
def test_reference_seeds_are_the_finite_differences_of_the_reference_loss(loss):
    """Away from the hinges and from zero (the drift term's kink): d (vec_scale * loss + B * mean drift) / d score."""
    rng = np.random.default_rng(5)
    B, par = 7, dict(inv_gbs=1 / 9, gp_coef=10.0, t=0.5, e_drift=1e-2, vec_scale=3.0)
    fs, rs, norms = rng.normal(size=B) * 2, rng.normal(size=B) * 2, rng.uniform(0.5, 2, size=B)
    for v, at in ((fs, (-1.0, 0.0)), (rs, (1.0, 0.0))):
        for a in at:
            v[np.abs(v - a) < 0.05] += 0.1

    def total(f, r):
        out = OR.np_d_loss(f, r, norms, loss, **par)
        lw = out["met"][2] - out["met"][3] - out["met"][4]
        return par["vec_scale"] * lw + B * out["met"][4]
    ref = OR.np_d_loss(fs, rs, norms, loss, **par)
    h = 1e-6
    for name, k in (("dfs", 0), ("drs", 1)):
        for b in range(B):
            hi, lo = [fs.copy(), rs.copy()], [fs.copy(), rs.copy()]
            hi[k][b] += h
            lo[k][b] -= h
            fd = (total(*hi) - total(*lo)) / (2 * h)
            assert abs(fd - ref[name][b]) < 1e-7, (name, b, fd, ref[name][b])
    g = OR.np_g_loss(fs, loss, par["inv_gbs"])
    for b in range(B):
        hi, lo = fs.copy(), fs.copy()
        hi[b] += h
        lo[b] -= h
        fd = (OR.np_g_loss(hi, loss, par["inv_gbs"])["met"][1] - OR.np_g_loss(lo, loss, par["inv_gbs"])["met"][1]) / (2 * h)
        assert abs(fd - g["ds"][b]) < 1e-8


def test_reference_hinge_subgradient_at_the_kink_is_zero():
    out = OR.np_d_loss(np.array([-1.0, -2.0, 0.0]), np.array([1.0, 2.0, 0.0]), None, "hinge", 0.5, 10.0, 1.0, 0.0, 2.0)
    assert list(out["dfs"]) == [0.0, 0.0, 1.0] and list(out["drs"]) == [0.0, 0.0, -1.0]
    assert out["met"][2] == (0 + 0 + 1 + 0 + 0 + 1) * 0.5 and out["met"][3] == 0 and out["met"][5] == 0


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_reference_seed_is_the_gradient_of_the_penalty_and_zero_target_never_divides(dtype):
    rng = np.random.default_rng(2)
    g = rng.normal(size=(3, 6)).astype(dtype)
    g[1] = 0
    n = np.sqrt((g.astype(np.float64) ** 2).sum(1)).astype(dtype)
    with np.errstate(all="raise"):
        z = OR.np_gp_seed(g, n, 0.7, 0.0, False, dtype)
    assert z.dtype == dtype and np.array_equal(z, dtype(0.7) * g) and (z[1] == 0).all()
    assert np.isnan(OR.np_gp_seed(g, n, 0.7, 0.5, False, dtype)[1]).all() and (OR.np_gp_seed(g, n, 0.7, 0.5, True, dtype)[1] == 0).all()
    if dtype is np.float64:
        # coef = 1 / 2: the seed is d sum((n - t)^2) / dg / 2 ... per sample d (n - t)^2 / dg = 2 (n - t) / n * g
        t, h = 0.5, 1e-6
        pen = lambda x: ((np.sqrt((x ** 2).sum(1)) - t) ** 2).sum()
        seed = OR.np_gp_seed(g, n, 2.0, t, True)
        for i, j in ((0, 0), (0, 5), (2, 3)):
            hi, lo = g.copy(), g.copy()
            hi[i, j] += h
            lo[i, j] -= h
            assert abs((pen(hi) - pen(lo)) / (2 * h) - seed[i, j]) < 1e-7
