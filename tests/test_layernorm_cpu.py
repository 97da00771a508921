"""layers.LayerNormalization without a GPU: the layer's surface and placement rules, the arithmetic of the kernels and of the
gradient penalty's second order in torch float64 against autograd, the order in which a critic step hands gradient slices to
the reducer, and what the compiler made of csrc/layernorm.hip."""
import contextlib
import importlib.util
import inspect
import io
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import blurred_gan_amd as bg
from blurred_gan_amd import engine, layers, models, ops

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
L = layers
DT = torch.float64


# ------------------------------------------------------------------ 1. the layer
def test_keras_defaults_and_variable_order():
    ln = L.LayerNormalization()
    assert (ln.kind, ln.axis, ln.epsilon, ln.center, ln.scale, ln.trainable) == ("layernorm", -1, 1e-3, True, True, True)
    assert L.LayerNormalization(axis=3, epsilon=1e-5).epsilon == 1e-5 and L.LayerNormalization(axis=[-1]).axis == -1
    specs = ln.var_specs((4, 4, 6))
    assert [(n, s, t) for n, s, t, _ in specs] == [("gamma", (6,), True), ("beta", (6,), True)]
    assert np.array_equal(specs[0][3](None), np.ones(6, np.float32)) and np.array_equal(specs[1][3](None), np.zeros(6, np.float32))
    assert ln.out_shape((4, 4, 6)) == (4, 4, 6)


def _stack(*between, head=True):
    ls = [L.Conv2D(8, 3, strides=2, padding="same", input_shape=(8, 8, 3)), *between]
    return L.Sequential(ls + ([L.Flatten(), L.Dense(1)] if head else []))


def test_variables_live_in_the_store_like_any_other():
    m = _stack(L.LayerNormalization(), L.LeakyReLU(), L.Dropout(0.3))
    m.build("cpu")
    names = [(type(l).__name__, n) for l, n, _, _, tr in m.store.entries if tr]
    assert names == [("Conv2D", "kernel"), ("Conv2D", "bias"), ("LayerNormalization", "gamma"), ("LayerNormalization", "beta"),
                     ("Dense", "kernel"), ("Dense", "bias")]
    assert m.count_params() == 3 * 3 * 3 * 8 + 8 + 8 + 8 + 4 * 4 * 8 + 1 and len(m.trainable_variables) == 6 == len(m.get_weights())
    ln = m.layers[1]
    assert ln.count_params() == 16 and bool((ln.vars["gamma"] == 1).all()) and bool((ln.vars["beta"] == 0).all())
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        m.summary()
    assert re.search(r"LayerNormalization\s+in=\(4, 4, 8\)\s+out=\(4, 4, 8\)\s+params=16\n", buf.getvalue()), buf.getvalue()
    net = m.net()
    st = net.stages[0]
    assert st.ln is ln and st.bn is None and st.act == "lrelu" and st.drop == 0.3 and not st.fusable_grad and net.has_ln
    assert net.store.train_range(st.lin, st.ln) == (0, 3 * 3 * 3 * 8 + 8 + 8 + 8)
    assert net._gp_kinds() == ["ln", "dense"]
    with pytest.raises(NotImplementedError, match="overwrites activations"):      # such a critic takes gp_second_order on the x-hat rows
        net.gp_second_order_merged(None, 0, 1)


@pytest.mark.parametrize("kw", [dict(axis=1), dict(axis=0), dict(axis=(1, 2, 3)), dict(axis=-2), dict(center=False), dict(scale=False)])
def test_unsupported_arguments_are_refused(kw):
    with pytest.raises(NotImplementedError):
        L.LayerNormalization(**kw)


def test_an_input_that_is_no_map_is_refused():
    with pytest.raises(NotImplementedError, match=r"\[H, W, C\]"):
        L.Sequential([L.Dense(4, input_shape=(3,)), L.LayerNormalization()])


def _refused(ls, match):
    m = L.Sequential(ls)
    m.build("cpu")
    with pytest.raises(NotImplementedError, match=match):
        m.net()


def test_placement_rules():
    conv = lambda **kw: L.Conv2D(8, 3, padding="same", **kw)
    first = dict(input_shape=(4, 4, 3))
    # supported: Conv2D with or without bias -> LayerNormalization -> LeakyReLU -> optional Dropout
    for ls in ([conv(**first), L.LayerNormalization(), L.LeakyReLU()],
               [conv(use_bias=False, **first), L.LayerNormalization(), L.LeakyReLU(), L.Dropout(0.3)]):
        m = L.Sequential(ls + [L.Flatten(), L.Dense(1)])
        m.build("cpu")
        assert m.net().stages[0].ln is ls[1]
    follow = "must directly follow a Conv2D"
    _refused([L.Dense(48, input_shape=(5,)), L.Reshape((4, 4, 3)), L.LayerNormalization(), L.LeakyReLU()], follow)
    _refused([L.Conv2DTranspose(8, 3, strides=2, padding="same", **first), L.LayerNormalization(), L.LeakyReLU()], follow)
    _refused([conv(**first), L.LeakyReLU(), L.AveragePooling2D(), L.LayerNormalization(), L.LeakyReLU(), L.Flatten(), L.Dense(1)], follow)
    _refused([conv(**first), L.UpSampling2D(), L.LayerNormalization(), L.LeakyReLU(), L.Flatten(), L.Dense(1)], follow)
    _refused([L.LayerNormalization(input_shape=(4, 4, 3)), conv()], follow)
    _refused([conv(**first), L.LeakyReLU(), L.LayerNormalization()], follow)
    both = "together with BatchNormalization"
    _refused([conv(**first), L.BatchNormalization(), L.LayerNormalization(), L.LeakyReLU()], both)
    _refused([conv(**first), L.LayerNormalization(), L.BatchNormalization(), L.LeakyReLU()], both)
    _refused([conv(**first), L.LayerNormalization(), L.Flatten(), L.Dense(1)], "must be followed by a LeakyReLU")
    _refused([conv(**first), L.LayerNormalization(), conv(), L.LeakyReLU()], "must be followed by a LeakyReLU")
    _refused([conv(activation="tanh", **first), L.LayerNormalization(), L.LeakyReLU()], "tanh")


def test_the_penalty_still_refuses_other_shapes_in_the_same_words():
    m = _stack(L.BatchNormalization(), L.LeakyReLU())
    m.build("cpu")
    with pytest.raises(NotImplementedError) as e:
        m.net()._gp_kinds()
    assert str(e.value) == engine._GP_SHAPE_MESSAGE and "LayerNorm" not in engine._GP_SHAPE_MESSAGE


@pytest.mark.parametrize("arch", ["tiny", "tiny_mnist", "mnist", "celeba64", "celeba128"])
@pytest.mark.parametrize("down", ["stride", "pool"])
def test_critic_builder(arch, down):
    plain, normed = models.DCGANDiscriminator(arch=arch, downsampling=down), models.DCGANDiscriminator(arch=arch, downsampling=down, normalization="layer")
    shapes = lambda m: [l.out_shape(s) for l, s in m.flat_layers() if l.kind != "layernorm"]
    assert shapes(plain) == shapes(normed) and normed.normalization == "layer" and plain.normalization is None
    kinds = [l.kind for l, _ in normed.flat_layers()]
    assert kinds.count("layernorm") == kinds.count("conv") == len(models._D[arch])
    assert all(kinds[i + 1] == "layernorm" and kinds[i + 2] == "lrelu" for i, k in enumerate(kinds) if k == "conv")
    count = lambda m: sum(int(np.prod(sh)) for l, s in m.flat_layers() for _, sh, _, _ in l.var_specs(s))
    assert count(normed) == count(plain) + 2 * sum(models._D[arch])
    with pytest.raises(ValueError):
        models.DCGANDiscriminator(arch=arch, normalization="batch")


def test_demos_take_the_switch():
    import demo_celeba
    import demo_mnist
    for demo in (demo_mnist, demo_celeba):
        assert demo.make_parser().parse_args([]).critic_norm == "none"
        assert demo.make_parser().parse_args(["--critic-norm", "layer"]).critic_norm == "layer"
        kinds = lambda m: [l.kind for l in m.layers]
        assert "layernorm" not in kinds(demo.DCGANDiscriminator())
        d = demo.DCGANDiscriminator(normalization="layer", downsampling="pool")
        assert kinds(d).count("layernorm") == kinds(d).count("conv") == kinds(d).count("avgpool")


# ------------------------------------------------------------------ 2. the formulas of the kernels against autograd, float64
EPS, ALPHA = 1e-3, 0.3


def _xhat(z):
    mu = z.mean(1, keepdim=True)
    r = 1.0 / torch.sqrt(((z - mu) ** 2).mean(1, keepdim=True) + EPS)
    return (z - mu) * r, r


def _M(y, xh, r):
    yc = y - y.mean(1, keepdim=True)
    return r * (yc - xh * (yc * xh).mean(1, keepdim=True))


def _source(u, zdot, xh, r, gamma):
    p = gamma * u - (gamma * u).mean(1, keepdim=True)
    q = zdot - zdot.mean(1, keepdim=True)
    A, Bq, D = (p * xh).mean(1, keepdim=True), (q * xh).mean(1, keepdim=True), (p * q).mean(1, keepdim=True)
    return -r ** 2 * (p * Bq + q * A + xh * (D - 3 * A * Bq))


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("R,C", [(5, 1), (4, 3), (7, 16), (3, 33)])
def test_the_four_formulas_equal_autograd(R, C):
    g = torch.Generator().manual_seed(R * 100 + C)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=DT)
    z = (rnd(R, C) * torch.logspace(-1, 1, R, dtype=DT).view(R, 1)).requires_grad_(True)
    gamma, beta = (1 + 0.2 * rnd(C)).requires_grad_(True), (0.1 * rnd(C)).requires_grad_(True)
    u, zdot = rnd(R, C), rnd(R, C).requires_grad_(True)
    # the normalisation in plain differentiable torch operations.  (F.layer_norm gives the same values -- asserted below -- and the
    # same first and second derivatives, which tests/ln_reference.py relies on and the penalty test below checks; but this test
    # differentiates the double-backward JVP once more, and through F.layer_norm's own backward formulas torch 2.10 returns a
    # different dT/dz than through these operations or through T written out directly.)
    n_of = lambda zz: gamma * _xhat(zz)[0] + beta
    xh, r = _xhat(z.detach())
    # forward
    assert _rel(gamma.detach() * xh + beta.detach(), n_of(z).detach()) < 1e-12
    assert _rel(n_of(z).detach(), torch.nn.functional.layer_norm(z.detach(), (C,), gamma.detach(), beta.detach(), EPS)) < 1e-12
    # backward: dz = M(gamma u), dgamma = sum u xh, dbeta = sum u
    dz, dg, db = torch.autograd.grad((u * n_of(z)).sum(), [z, gamma, beta])
    assert _rel(_M(gamma.detach() * u, xh, r), dz) < 1e-12 or C == 1
    assert _rel((u * xh).sum(0), dg) < 1e-12 or C == 1
    assert _rel(u.sum(0), db) < 1e-12
    # tangent: the JVP of n along zdot is gamma M(zdot)
    _, tan = torch.autograd.functional.jvp(n_of, z, zdot, create_graph=True)
    assert _rel(gamma.detach() * _M(zdot.detach(), xh, r), tan.detach()) < 1e-12 or C == 1
    # source: T = <u, gamma M(zdot)>; dT/dzdot = M(gamma u), dT/dgamma = sum u M(zdot), dT/dz = s
    dzdot, dgam, s = torch.autograd.grad((u * tan).sum(), [zdot, gamma, z])
    assert _rel(_M(gamma.detach() * u, xh, r), dzdot) < 1e-12 or C == 1
    assert _rel((u * _M(zdot.detach(), xh, r)).sum(0), dgam) < 1e-12 or C == 1
    assert _rel(_source(u, zdot.detach(), xh, r, gamma.detach()), s) < 1e-12 or C == 1
    # the same dT/dz with T written out, no JVP involved
    zz = z.detach().clone().requires_grad_(True)
    xh_z, r_z = _xhat(zz)
    direct, = torch.autograd.grad((u * gamma.detach() * _M(zdot.detach(), xh_z, r_z)).sum(), zz)
    assert _rel(s, direct) < 1e-12 or C == 1
    if C == 1:       # one channel: xh = 0 and M = 0 identically; autograd's values are rounding noise around that zero
        for got in (dz, dg, tan.detach(), dzdot, dgam, s):
            assert float(got.abs().max()) < 1e-12
        for mine in (_M(gamma.detach() * u, xh, r), _source(u, zdot.detach(), xh, r, gamma.detach())):
            assert float(mine.abs().max()) == 0.0


def test_the_penalty_gradient_assembled_by_the_three_passes_equals_autograd():
    """A critic with two LayerNormalization stages (1x1 convolutions: a pixel's row times a matrix): the gradient of the penalty
    for every parameter, assembled exactly as engine.Net does it -- (1) first-order backward keeping u_i and zeta_i, (2)
    linearised forward with the LN tangent, filter gradients against zeta_i, dgamma_i += sum u_i M(zdot_i), s_i, (3) source
    backward from the top-most LN stage -- against autograd.grad of the penalty, to 1e-10."""
    g = torch.Generator().manual_seed(11)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=DT)
    B, P, C0, C1, C2 = 3, 4, 3, 6, 5                  # samples, pixels per sample, channels
    alpha = 0.3                                       # float64: a float32 0.3 would cost 1e-8
    W1, b1, g1, be1 = 0.5 * rnd(C0, C1), 0.1 * rnd(C1), 1 + 0.2 * rnd(C1), 0.1 * rnd(C1)
    W2, b2, g2, be2 = 0.5 * rnd(C1, C2), 0.1 * rnd(C2), 1 + 0.2 * rnd(C2), 0.1 * rnd(C2)
    wd = rnd(P * C2)
    params = [W1, b1, g1, be1, W2, b2, g2, be2, wd]
    x = rnd(B * P, C0)
    coef = 10.0

    # ---- autograd
    leaves = [p.clone().requires_grad_(True) for p in params]
    xa = x.clone().requires_grad_(True)

    def critic(a, prm):
        w1, c1, ga1, bb1, w2, c2, ga2, bb2, head = prm
        for w, c, ga, bb in ((w1, c1, ga1, bb1), (w2, c2, ga2, bb2)):
            zz = a @ w + c
            a = torch.nn.functional.leaky_relu(ga * torch.nn.functional.layer_norm(zz, zz.shape[-1:], None, None, EPS) + bb, alpha)
        return a.reshape(B, -1) @ head

    gx, = torch.autograd.grad(critic(xa, leaves).sum(), xa, create_graph=True)
    pen = coef * ((gx.reshape(B, -1).norm(dim=1) - 1.0) ** 2).mean()
    want = torch.autograd.grad(pen, leaves, allow_unused=True)

    # ---- the three passes, no autograd
    lr = lambda n: torch.where(n > 0, torch.ones_like(n), torch.full_like(n, alpha))
    a0 = x
    z1 = a0 @ W1 + b1
    xh1, r1 = _xhat(z1)
    n1 = g1 * xh1 + be1
    a1 = torch.where(n1 > 0, n1, alpha * n1)
    z2 = a1 @ W2 + b2
    xh2, r2 = _xhat(z2)
    n2 = g2 * xh2 + be2
    # (1) first-order backward with seed 1: u_i, zeta_i
    u2 = wd.view(1, P, C2).expand(B, P, C2).reshape(B * P, C2) * lr(n2)
    zeta2 = _M(g2 * u2, xh2, r2)
    u1 = (zeta2 @ W2.T) * lr(n1)
    zeta1 = _M(g1 * u1, xh1, r1)
    grad_x = (zeta1 @ W1.T).reshape(B, -1)
    norm = grad_x.norm(dim=1, keepdim=True)
    v0 = (coef * 2.0 / B * (norm - 1.0) / norm * grad_x).reshape(B * P, C0)
    got = [torch.zeros_like(p) for p in params]
    dW1, db1, dg1, dbe1, dW2, db2, dg2, dbe2, dwd = got
    # (2) linearised forward
    zd1 = v0 @ W1
    dW1 += v0.T @ zeta1
    t1 = lr(n1) * g1 * _M(zd1, xh1, r1)
    dg1 += (u1 * _M(zd1, xh1, r1)).sum(0)
    s1 = _source(u1, zd1, xh1, r1, g1)
    zd2 = t1 @ W2
    dW2 += t1.T @ zeta2
    t2 = lr(n2) * g2 * _M(zd2, xh2, r2)
    dg2 += (u2 * _M(zd2, xh2, r2)).sum(0)
    s2 = _source(u2, zd2, xh2, r2, g2)
    dwd += t2.reshape(B, -1).sum(0)
    # (3) source backward from the top-most LN stage: primal inputs, beta = 1
    dW2 += a1.T @ s2
    db2 += s2.sum(0)
    uu = (s2 @ W2.T) * lr(n1)
    dg1 += (uu * xh1).sum(0)
    dbe1 += uu.sum(0)
    lam1 = _M(g1 * uu, xh1, r1) + s1
    dW1 += a0.T @ lam1
    db1 += lam1.sum(0)
    for name, a, b in zip("W1 b1 gamma1 beta1 W2 b2 gamma2 beta2 head".split(), got, want):
        b = torch.zeros_like(a) if b is None else b
        err = float((a - b).abs().max())
        print(f"{name}: max|err| {err:.2e}, max|ref| {float(b.abs().max()):.2e}")
        assert err <= 1e-10 * max(1.0, float(b.abs().max())), name
    assert want[7] is None or float(want[7].abs().max()) < 1e-12      # the top stage's beta: the penalty does not depend on it


# ------------------------------------------------------------------ 3. what a critic step enqueues, and when slices go to the reducer
_spec = importlib.util.spec_from_file_location("make_engine_trace", os.path.join(HERE, "golden", "make_engine_trace.py"))
maker = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(maker)
LN_RETURNS = {"fwd": "a", "bwd": "dz", "tangent": "vout", "gp_source": "s"}


class _Recorder:
    """Launches as (name, arguments) and reducer hand-overs as ("ready", (lo, hi)), in the order the step enqueues them."""

    def __init__(self):
        self.events = []

    def wrap(self, name, real, ret):
        sig = inspect.signature(real)

        def rec(*a, **k):
            b = sig.bind(*a, **k)
            b.apply_defaults()
            args = dict(b.arguments)
            if "counter" in args:
                args["offset"] = ops._draw_offset(args["out"], args["offset"], args.pop("counter"))
            self.events.append((name, args))
            return args[ret] if ret else None
        return rec

    def ready(self, lo, hi):
        self.events.append(("ready", (int(lo), int(hi))))

    def finish(self):
        self.events.append(("finish", ()))


@contextlib.contextmanager
def recording(rec):
    saved = []

    def patch(obj, name, new):
        saved.append((obj, name, obj.__dict__[name] if isinstance(obj, type) else getattr(obj, name)))
        setattr(obj, name, new)

    for name, ret in maker.RETURNS.items():
        patch(ops, name, rec.wrap(name, getattr(ops, name), ret))
    for name, ret in LN_RETURNS.items():
        patch(ops.layernorm, name, staticmethod(rec.wrap("layernorm." + name, getattr(ops.layernorm, name), ret)))
    patch(bg.dist, "GradReducer", lambda *a, **k: rec)
    patch(layers, "default_device", lambda: torch.device("cpu"))
    try:
        yield rec
    finally:
        for obj, name, old in reversed(saved):
            setattr(obj, name, old)


def _grad_writes(args, grad):
    """[lo, hi) ranges of the flat gradient buffer among a launch's tensor arguments (the launches only ever write there)."""
    out = []
    for v in args.values():
        if isinstance(v, torch.Tensor) and v.numel() and v.untyped_storage().data_ptr() == grad.untyped_storage().data_ptr():
            out.append((v.storage_offset(), v.storage_offset() + v.numel()))
    return out


def _cpu_gan(cls=None, blur=False, down="stride", **kw):
    cls = cls or (bg.BlurredWGANGP if blur else bg.WGANGP)
    bg.layers.set_seed(3)
    gen, disc = models.DCGANGenerator(arch="tiny"), models.DCGANDiscriminator(arch="tiny", downsampling=down, normalization="layer")
    gen.build("cpu"), disc.build("cpu")
    hp = cls.HyperParameters(batch_size=2, global_batch_size=2, **({"initial_blur_std": 0.9} if blur else {}))
    return cls(gen, disc, hp, bg.TrainingConfig(log_dir=os.devnull), step_replay=False, **kw)


D_STEP_CONFIGS = {"merged": {}, "merged_separate_wgrad": dict(merge_gp_filter_gradients=False), "unmerged": dict(merge_critic_passes=False)}


@pytest.mark.parametrize("config", sorted(D_STEP_CONFIGS))
@pytest.mark.parametrize("variant", ["plain", "blur", "pool"])
def test_no_slice_goes_to_the_reducer_before_its_last_write(config, variant):
    maker.ensure_library(ROOT)
    rec = _Recorder()
    with recording(rec):
        gan = _cpu_gan(blur=variant == "blur", down="pool" if variant == "pool" else "stride", **D_STEP_CONFIGS[config])
        gan.train_on_batch(np.zeros((2, 8, 8, 3), np.float32))
    D = gan.discriminator.net()
    grad = D.store.grad
    ev = rec.events[:[n for n, _ in rec.events].index("finish") + 1]         # the critic step, up to its reducer's finish()
    names = [n for n, _ in ev]
    # every D-step configuration takes the separate second-order route: the tangent, the source and the source backward
    n_ln = sum(st.ln is not None for st in D.stages)
    assert n_ln == 2 and names.count("layernorm.tangent") == n_ln == names.count("layernorm.gp_source")
    first_source = names.index("layernorm.gp_source")
    last_source = len(names) - 1 - names[::-1].index("layernorm.gp_source")
    assert names[last_source:].count("layernorm.bwd") == n_ln - 1          # the source backward: every LN stage below the top one
    handed = [(k, a) for k, (n, a) in enumerate(ev) if n == "ready"]
    assert handed and names.index("finish") > handed[-1][0]
    for k, (lo, hi) in handed:
        late = [(names[j], w) for j in range(k + 1, len(ev)) if names[j] not in ("ready", "finish", "adam")
                for w in _grad_writes(ev[j][1], grad) if w[0] < hi and w[1] > lo]
        assert not late, f"[{lo}, {hi}) handed over at event {k}, written again by {late}"
    # each layer's slice is handed over exactly once, and the LN layers' only behind the source backward's launches
    ranges = [D._train_range(st) for st in D.stages if st.kind not in engine.RESAMPLE]
    assert sorted(a for _, a in handed) == sorted(ranges)
    for st in D.stages:
        if st.ln is not None:
            k = next(k for k, a in handed if a == D._train_range(st))
            assert k > last_source and k > first_source
    # the first-order backward keeps u for exactly the x-hat rows
    bwd = [a for n, a in ev[:first_source] if n == "layernorm.bwd" and a["u_out"] is not None]
    assert len(bwd) == n_ln and all(a["u_out"].shape[0] == 2 for a in bwd)


def test_the_generator_step_and_plain_wgan_take_the_first_order_path_only():
    maker.ensure_library(ROOT)
    rec = _Recorder()
    with recording(rec):
        gan = _cpu_gan(cls=bg.WGAN)
        gan.train_on_batch(np.zeros((2, 8, 8, 3), np.float32))
    names = [n for n, _ in rec.events]
    assert "layernorm.tangent" not in names and "layernorm.gp_source" not in names
    bwd = [a for n, a in rec.events if n == "layernorm.bwd"]
    assert len(bwd) == 4 and all(a["u_out"] is None and a["addend"] is None for a in bwd)
    assert [a["dgamma"] is not None for a in bwd] == [True, True, False, False]       # D-step, then the G-step's need_dw=False form
    fwd = [a for n, a in rec.events if n == "layernorm.fwd"]
    assert [a["keep"] is not None for a in fwd] == [True, True, False, False]          # Dropout behind LN in training, none in the G-step


def test_a_step_without_layernorm_enqueues_no_layernorm_launch():
    maker.ensure_library(ROOT)
    rec = _Recorder()
    with recording(rec):
        bg.layers.set_seed(3)
        gen, disc = models.DCGANGenerator(arch="tiny"), models.DCGANDiscriminator(arch="tiny")
        gen.build("cpu"), disc.build("cpu")
        gan = bg.WGANGP(gen, disc, bg.WGANGP.HyperParameters(batch_size=2, global_batch_size=2), bg.TrainingConfig(log_dir=os.devnull), step_replay=False)
        gan.train_on_batch(np.zeros((2, 8, 8, 3), np.float32))
    assert not [n for n, _ in rec.events if n.startswith("layernorm.")]
    assert "blur_grad" not in gan.discriminator.net().context(6, "fr3", drop_rows=4)._extra


# ------------------------------------------------------------------ 4. the code objects
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_kernels_use_no_private_memory_and_move_float4(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = tmp_path / "layernorm.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-ffp-contract=off", "-w", "--cuda-device-only", "-S",
                    os.path.join(ROOT, "blurred-gan_amd", "csrc", "layernorm.hip"), "-o", str(out)], check=True)
    isa = out.read_text()
    kernels = list(re.finditer(r"\.name:\s+(\S*_kernel\S*)\n(.*?)\.wavefront_size", isa, flags=re.S))
    names = [m.group(1) for m in kernels]
    # forward, backward, tangent, source: 8 routes each (float4 / scalar x 1, 2, 4 units in registers + the chunked sweep), + the finish
    assert len(names) == 33 and sum("ln_apply_kernel" in n for n in names) == 16, names
    for m in kernels:
        for key in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
            v = re.search(r"\." + key + r":\s+(\d+)", m.group(2))
            assert v and int(v.group(1)) == 0, (m.group(1), key)
    for name in names:
        if "Li4ELi" in name:          # <MODE, VEC = 4, ...>: the float4 routes
            body = re.search(r"^" + re.escape(name) + r":(.*?)s_endpgm", isa, flags=re.S | re.M).group(1)
            assert "global_load_dwordx4" in body and "global_store_dwordx4" in body, name
