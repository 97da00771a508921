"""layers.StyleModulation without a GPU: the wrapper's surface, the generator keyword of models.py (and that the "batch" and "pixel"
stacks are what they were), every refusal with the rule in its message, what a network with modulated stages enqueues, and the
float64 reference of tests/modconv_reference.py against StyleGAN2's definition (per-sample modulated and demodulated weights), its
written-out backward against autograd, and autograd against finite differences."""
import contextlib
import importlib.util
import inspect
import os

import numpy as np
import pytest
import torch

import blurred_gan_amd as bg
from blurred_gan_amd import layers, models, ops
import modconv_reference as MC

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
L = layers
RULE = "StyleModulation wraps a Conv2D, a Conv2DTranspose or an EqualizedLearningRate around one of them"

_spec = importlib.util.spec_from_file_location("make_engine_trace", os.path.join(HERE, "golden", "make_engine_trace.py"))
maker = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(maker)


# ------------------------------------------------------------------ 1. the wrapper
def _entries(m):
    m.build("cpu")
    own = {id(l) for l in m._own_layers()}
    return [(type(l).__name__, n, tuple(shape), tr) for (l, n, _, shape, tr) in m.store.entries if id(l) in own]


def _stack(mod, L_=7, first=None):
    return L.Sequential([L.Dense(48, input_shape=(L_,)), L.Reshape((4, 4, 3)), L.LeakyReLU(), L.PixelNormalization()] + list(mod))


def test_wrapper_surface():
    bg.set_seed(5)
    conv = L.Conv2D(8, 3, padding="same")
    m = L.StyleModulation(conv)
    assert m.kind == "conv" and m.demodulate and m.epsilon == 1e-8 and m.filters == 8 and m.k == 3 and m.stride == 1 and m.use_bias
    assert m.out_shape((4, 4, 3)) == (4, 4, 8) and m.vars is conv.vars
    t = L.StyleModulation(L.EqualizedLearningRate(L.Conv2DTranspose(8, 3, strides=2, padding="same")))
    assert t.kind == "convT" and t.out_shape((4, 4, 3)) == (8, 8, 8) and t.vars is t.layer.vars is t.layer.layer.vars
    with pytest.raises(NotImplementedError, match="no style source"):          # L is the model's: unknown outside one
        m.var_specs((4, 4, 3))
    net_in = 7
    model = _stack([m, L.LeakyReLU(), t, L.LeakyReLU(),
                    L.StyleModulation(L.Conv2D(3, 3, padding="same", use_bias=False, activation="tanh"), demodulate=False)], net_in)
    ent = _entries(model)
    assert m.style_dim == t.style_dim == net_in
    assert ent[2:] == [("StyleModulation", "kernel", (3, 3, 3, 8), True), ("StyleModulation", "bias", (8,), True),
                       ("StyleModulation", "style_kernel", (7, 3), True), ("StyleModulation", "style_bias", (3,), True),
                       ("StyleModulation", "kernel", (3, 3, 8, 8), True), ("StyleModulation", "bias", (8,), True),
                       ("StyleModulation", "style_kernel", (7, 8), True), ("StyleModulation", "style_bias", (8,), True),
                       ("StyleModulation", "kernel", (3, 3, 8, 3), True),
                       ("StyleModulation", "style_kernel", (7, 8), True), ("StyleModulation", "style_bias", (8,), True)]
    A, a = m.vars["style_kernel"].numpy(), m.vars["style_bias"].numpy()
    lim = np.sqrt(6.0 / (7 + 3))
    assert np.array_equal(a, np.ones(3, np.float32)) and np.abs(A).max() <= lim and np.abs(A).max() > 0.3 * lim and A.std() > 0
    assert np.array_equal(m.vars["bias"].numpy(), np.zeros(8, np.float32))
    # the wrapped EqualizedLearningRate keeps its rule: N(0, 1) kernel, coefficient from the fan-in
    assert abs(t.coefficient - np.sqrt(2) / np.sqrt(9 * 8)) < 1e-7 and 0.7 < t.vars["kernel"].numpy().std() < 1.3
    net = model.net()
    assert [st.mod is not None for st in net.stages] == [False, True, True, True] and net.has_mod
    assert net.eqlr_layers == [t.layer] and net.plain_conv_layers == [m, net.stages[3].lin]
    # the style variables lie inside their stage's slice of the trainable buffer
    for st in net.stages[1:]:
        lo, hi = net._train_range(st)
        offs = [o for (l, n, o, _, _) in model.store.entries if l is st.lin]
        assert lo == min(offs) and all(lo <= o < hi for o in offs)
    with pytest.raises(ValueError, match="epsilon"):
        L.StyleModulation(L.Conv2D(8, 3, padding="same"), epsilon=0.0)


def test_parameter_count_of_the_tiny_style_generator():
    g = models.DCGANGenerator(arch="tiny", normalization="style")
    g.build("cpu")
    L_ = 10
    dense = 10 * 128 + 128
    c1 = 5 * 5 * 32 * 32 + 32 + (L_ * 32 + 32)
    c2 = 5 * 5 * 16 * 32 + 16 + (L_ * 32 + 32)
    c3 = 5 * 5 * 16 * 16 + 16 + (L_ * 16 + 16)
    rgb = 5 * 5 * 16 * 3 + (L_ * 16 + 16)
    assert g.count_params() == dense + c1 + c2 + c3 + rgb == 48528
    n = models.DCGANGenerator(arch="tiny", normalization="style", noise=True)
    n.build("cpu")
    assert n.count_params() == 48528 + 3


@pytest.mark.parametrize("up", ["transpose", "resize", "filtered"])
@pytest.mark.parametrize("kw", [{}, dict(noise=True), dict(equalized_lr=True), dict(normalize_latents=True)], ids=lambda k: "_".join(k) or "plain")
def test_style_generator_builder(up, kw):
    g = models.DCGANGenerator(arch="tiny", normalization="style", upsampling=up, **kw)
    g.build("cpu")
    names = [type(l).__name__ for l, _ in g.flat_layers()]
    head = (["PixelNormalization"] if kw.get("normalize_latents") else []) + ["EqualizedLearningRate" if kw.get("equalized_lr") else "Dense",
                                                                              "Reshape", "LeakyReLU", "PixelNormalization"]
    tail = []
    for stride in (1, 2, 2):
        if stride == 2 and up != "transpose":
            tail.append("UpSampling2D" if up == "resize" else "FilteredUpSampling2D")
        tail += ["StyleModulation"] + (["NoiseInjection"] if kw.get("noise") else []) + ["LeakyReLU"]
    assert names == head + tail + ["StyleModulation"]
    mods = [l for l, _ in g.flat_layers() if isinstance(l, L.StyleModulation)]
    assert [m.demodulate for m in mods] == [True, True, True, False] and [m.use_bias for m in mods] == [True, True, True, False]
    assert mods[-1].activation == "tanh" and all(m.style_dim == 10 for m in mods)
    assert all(isinstance(m.layer, L.EqualizedLearningRate) == bool(kw.get("equalized_lr")) for m in mods)
    if kw.get("equalized_lr"):
        assert [round(m.layer.gain, 6) for m in mods] == [round(np.sqrt(2), 6)] * 3 + [1.0]
        assert isinstance(g.flat_layers()[0][0], L.EqualizedLearningRate)          # the Dense, as in every equalised stack
    net = g.net()
    assert net.has_mod and len(net.mod_layers) == 4 and (net.latent_pn is not None) == bool(kw.get("normalize_latents"))


def test_batch_and_pixel_stacks_are_what_they_were():
    """Written out by hand for "tiny" (latents 10, 2x2x32 base, transposed convs 32 / 16 / 16, a 3-channel tanh conv, 5x5 kernels)."""
    k = lambda n, *s: (n, "kernel", s, True)
    bn = lambda c: [("BatchNormalization", "gamma", (c,), True), ("BatchNormalization", "beta", (c,), True),
                    ("BatchNormalization", "moving_mean", (c,), False), ("BatchNormalization", "moving_variance", (c,), False)]
    b = lambda n, c: (n, "bias", (c,), True)
    T, C, D = "Conv2DTranspose", "Conv2D", "Dense"
    g = models.DCGANGenerator(arch="tiny")
    assert [type(l).__name__ for l, _ in g.flat_layers()] == [
        D, "BatchNormalization", "LeakyReLU", "Reshape", T, "BatchNormalization", "LeakyReLU", T, "BatchNormalization", "LeakyReLU",
        T, "BatchNormalization", "LeakyReLU", C]
    assert _entries(g) == [k(D, 10, 128)] + bn(128) + [k(T, 5, 5, 32, 32)] + bn(32) + [k(T, 5, 5, 16, 32)] + bn(16) + [k(T, 5, 5, 16, 16)] + bn(16) \
        + [k(C, 5, 5, 16, 3)]
    p = models.DCGANGenerator(arch="tiny", normalization="pixel")
    assert [type(l).__name__ for l, _ in p.flat_layers()] == [
        D, "Reshape", "LeakyReLU", "PixelNormalization", T, "LeakyReLU", "PixelNormalization", T, "LeakyReLU", "PixelNormalization",
        T, "LeakyReLU", "PixelNormalization", C]
    assert _entries(p) == [k(D, 10, 128), b(D, 128), k(T, 5, 5, 32, 32), b(T, 32), k(T, 5, 5, 16, 32), b(T, 16), k(T, 5, 5, 16, 16), b(T, 16),
                           k(C, 5, 5, 16, 3)]
    for m in (g, p):
        assert not m.net().has_mod and m.net().mod_layers == []
    n = models.DCGANGenerator(arch="tiny", normalization="pixel", noise=True)
    assert [type(l).__name__ for l, _ in n.flat_layers()].count("NoiseInjection") == 3


# ------------------------------------------------------------------ 2. refusals
def _refused(build, match=RULE, exc=NotImplementedError):
    with pytest.raises(exc, match=match):
        m = build()
        if isinstance(m, L.Sequential):
            m.build("cpu")
            m.net()


def test_refusals_carry_the_rule():
    SM, LR = L.StyleModulation, L.LeakyReLU
    conv = lambda **kw: L.Conv2D(8, 3, padding="same", **kw)
    tanh = lambda **kw: L.Conv2D(3, 3, padding="same", activation="tanh", **kw)
    _refused(lambda: SM(L.Dense(8)))                                                           # a Dense
    _refused(lambda: SM(L.EqualizedLearningRate(L.Dense(8))))
    _refused(lambda: SM(L.SpectralNormalization(conv())))                                      # SpectralNormalization, either nesting
    with pytest.raises(NotImplementedError):
        L.SpectralNormalization(SM(conv()))
    with pytest.raises(NotImplementedError):
        L.EqualizedLearningRate(SM(conv()))                                                    # only the one nesting
    _refused(lambda: SM(LR()))
    _refused(lambda: SM(tanh(use_bias=False)), match="demodulate=True in a stage with tanh")
    _refused(lambda: SM(tanh(use_bias=False)))
    _refused(lambda: SM(conv(), demodulate=False), match="demodulate=False with a bias")
    _refused(lambda: SM(conv(), demodulate=False))
    # in a network
    _refused(lambda: _stack([SM(conv()), L.BatchNormalization(), LR()]))
    _refused(lambda: _stack([SM(conv()), L.BatchNormalization(), LR()]), match="BatchNormalization in the stage of a StyleModulation")
    _refused(lambda: _stack([SM(conv()), L.LayerNormalization(), LR()]))
    _refused(lambda: _stack([SM(conv()), LR(), L.Dropout(0.3)]))
    _refused(lambda: _stack([SM(conv()), LR(), L.PixelNormalization()]))
    # a first stage: the only style source is the [L] input
    _refused(lambda: L.Sequential([SM(conv(input_shape=(4, 4, 3))), LR()]))
    _refused(lambda: L.Sequential([SM(conv(input_shape=(4, 4, 3))), LR()]), match="no style source")
    # a critic containing the layer (its input is an image: no style source), and WGAN on a built one
    _refused(lambda: L.Sequential([L.Conv2D(8, 3, strides=2, padding="same", input_shape=(8, 8, 3)), LR(), SM(conv()), LR(), L.Flatten(), L.Dense(1)]))
    # the gradient at the input, and the penalty's second order
    m = _stack([SM(conv()), LR()])
    m.build("cpu")
    net = m.net()
    with pytest.raises(NotImplementedError, match="dL/dw"):
        net.backward(None, None, need_dx=True)
    for call in (lambda: net.gp_second_order(None, None), lambda: net.gp_second_order_merged(None, 0, 2)):
        with pytest.raises(NotImplementedError, match="StyleModulation in a critic under the gradient penalty is not built"):
            call()
    # accepted: with a NoiseInjection, without an activation, behind a resampling stage
    ok = _stack([SM(conv()), L.NoiseInjection(), LR(), L.UpSampling2D(), SM(conv()), SM(tanh(use_bias=False), demodulate=False)])
    ok.build("cpu")
    assert [st.mod is not None for st in ok.net().stages] == [False, True, False, True, True] and ok.net().stages[3].act is None


def test_wgan_refuses_a_critic_with_the_layer():
    critic = L.Sequential([L.Dense(192, use_bias=False, input_shape=(192,)), L.BatchNormalization(), L.LeakyReLU(), L.Reshape((8, 8, 3)),
                           L.StyleModulation(L.Conv2D(8, 3, strides=2, padding="same")), L.LeakyReLU(), L.Flatten(), L.Dense(1)])
    critic.build("cpu")
    gen = models.DCGANGenerator(arch="tiny")
    gen.build("cpu")
    for cls in (bg.WGAN, bg.WGANGP):
        with pytest.raises(NotImplementedError, match="StyleModulation in the discriminator"):
            cls(gen, critic, cls.HyperParameters(batch_size=2, global_batch_size=2), bg.TrainingConfig(log_dir=os.devnull))


def test_models_refusals_and_noise_rule():
    with pytest.raises(ValueError, match="spectral_norm=True"):
        models.DCGANGenerator(arch="tiny", normalization="style", spectral_norm=True)
    with pytest.raises(ValueError, match="or 'style'"):
        models.DCGANGenerator(arch="tiny", normalization="group")
    with pytest.raises(ValueError, match="noise=True needs normalization='pixel' or 'style'"):
        models.DCGANGenerator(arch="tiny", noise=True)
    assert 'normalization="style"' in models.__doc__


def test_demos_take_the_choice():
    for demo in ("demo_celeba.py", "demo_mnist.py"):
        src = open(os.path.join(ROOT, demo)).read()
        assert 'choices=["batch", "pixel", "style"]' in src


# ------------------------------------------------------------------ 3. what a network with modulated stages enqueues
class _Recorder:
    """Launches as (name, arguments), in the order they are enqueued."""

    def __init__(self):
        self.events = []

    def wrap(self, name, real, ret):
        sig = inspect.signature(real)

        def rec(*a, **k):
            b = sig.bind(*a, **k)
            b.apply_defaults()
            args = dict(b.arguments)
            self.events.append((name, args))
            return args[ret] if ret else None
        return rec

    def ready(self, lo, hi):
        self.events.append(("ready", (int(lo), int(hi))))


MOD_RETURNS = {"scale": "out", "dot": "out", "wsq": "q", "wsq_grad": "dw", "demod": "d", "demod_bwd": None}


@contextlib.contextmanager
def recording(rec):
    saved = []

    def patch(obj, name, new):
        saved.append((obj, name, obj.__dict__[name] if isinstance(obj, type) else getattr(obj, name)))
        setattr(obj, name, new)

    for name, ret in maker.RETURNS.items():
        patch(ops, name, rec.wrap(name, getattr(ops, name), ret))
    for name, ret in MOD_RETURNS.items():
        patch(ops.modconv, name, staticmethod(rec.wrap(f"modconv.{name}", getattr(ops.modconv, name), ret)))
    patch(ops.modconv, "dot_workspace_bytes", staticmethod(lambda B, P, Cc: 0))
    for name, ret in {"fwd": "y", "bwd": "dz"}.items():
        patch(ops.pixelnorm, name, staticmethod(rec.wrap(f"pixelnorm.{name}", getattr(ops.pixelnorm, name), ret)))
    sig = inspect.signature(ops.epilogue)

    def epilogue(*a, **k):      # the descriptor as the keywords it was made from
        b = sig.bind(*a, **k)
        b.apply_defaults()
        return dict(b.arguments)
    patch(ops, "epilogue", epilogue)
    patch(ops, "conv2d_stats_rows", lambda epi: 0)
    patch(layers, "default_device", lambda: torch.device("cpu"))
    try:
        yield rec
    finally:
        for obj, name, old in reversed(saved):
            setattr(obj, name, old)


def test_launch_record_of_a_two_stage_network():
    """Dense block, a demodulated transposed convolution, the modulated tanh convolution: one forward and one backward."""
    maker.ensure_library(ROOT)
    bg.layers.set_seed(3)
    B, Ls = 2, 6
    t = L.StyleModulation(L.Conv2DTranspose(8, 3, strides=2, padding="same"))
    rgb = L.StyleModulation(L.Conv2D(3, 3, padding="same", use_bias=False, activation="tanh"), demodulate=False)
    m = _stack([t, L.LeakyReLU(0.2), rgb], Ls)
    m.build("cpu")
    net, store = m.net(), m.store
    s1, s2 = net.stages[1], net.stages[2]
    rec = _Recorder()
    with recording(rec):
        ctx = net.context(B, "test")
        z = torch.zeros(B, Ls)
        for training in (False, True):          # the same launches in inference and in training
            del rec.events[:]
            store.tr_dirty = True
            out = net.forward(ctx, z, training=training)
            ev = list(rec.events)
            names = [n for n, _ in ev]
            # derived weights first: Q of the one demodulating layer, one launch, behind the transposed copies
            assert names.count("modconv.wsq") == 1 and names.index("transpose_last2_batched") < names.index("modconv.wsq") < names.index("gemm")
            q = ev[names.index("modconv.wsq")][1]
            assert q["w"] is t.vars["kernel"] and q["q"] is store.mod_q(t) and (q["taps"], q["I"], q["O"], q["transposed"]) == (9, 3, 8, True)
            k0 = names.index("pixelnorm.fwd")
            assert names[k0 + 1:] == ["gemm", "modconv.scale", "conv2d_bwd_data", "modconv.demod", "modconv.scale", "gemm", "modconv.scale", "conv2d_fwd"]
            g1, x1, c1, d1, y1, g2, x2, c2 = [a for _, a in ev[k0 + 1:]]
            assert g1["A"].data_ptr() == z.data_ptr() and g1["Bm"] is t.vars["style_kernel"] and g1["bias"] is t.vars["style_bias"] and g1["Cm"] is ctx.mod_s[1]
            assert (g1["M"], g1["N"], g1["K"]) == (B, 3, Ls)
            assert x1["x"].data_ptr() == ctx.a[0].data_ptr() and x1["v"] is ctx.mod_s[1] and x1["out"] is ctx.mod_xs[1]
            assert (x1["B"], x1["P"], x1["Cc"], x1["bias"], x1["lrelu_alpha"]) == (B, 16, 3, None, 1.0)
            assert c1["dy"] is ctx.mod_xs[1] and c1["dx"] is ctx.z[1] and c1["epi"]["mode"] == ops.EPI_NONE and c1["epi"]["bias"] is None
            assert d1["s"] is ctx.mod_s[1] and d1["q"] is store.mod_q(t) and d1["d"] is ctx.mod_d[1] and (d1["B"], d1["I"], d1["O"]) == (B, 3, 8)
            assert d1["eps"] == 1e-8
            assert y1["x"] is ctx.z[1] and y1["v"] is ctx.mod_d[1] and y1["out"] is ctx.a[1] and y1["bias"] is t.vars["bias"]
            assert (y1["B"], y1["P"], y1["Cc"], y1["lrelu_alpha"]) == (B, 64, 8, 0.2)
            assert g2["A"].data_ptr() == z.data_ptr() and g2["Bm"] is rgb.vars["style_kernel"] and g2["Cm"] is ctx.mod_s[2] and (g2["M"], g2["N"], g2["K"]) == (B, 8, Ls)
            assert x2["x"].data_ptr() == ctx.a[1].data_ptr() and x2["out"] is ctx.mod_xs[2] and (x2["B"], x2["P"], x2["Cc"]) == (B, 64, 8)
            assert c2["x"] is ctx.mod_xs[2] and c2["y"] is ctx.a[2] and c2["epi"]["mode"] == ops.EPI_TANH and out is ctx.a[2]
            assert ctx.mod_d[2] is None and ctx.z[2] is None
        # clean weights: no refresh
        del rec.events[:]
        net.forward(ctx, z)
        assert "modconv.wsq" not in [n for n, _ in rec.events]
        del rec.events[:]
        dout = torch.zeros(B, 8, 8, 3)
        assert net.backward(ctx, dout, need_dx=False, need_dw=True, beta=0.5, scale=2.0, reducer=rec) is None
        ev = list(rec.events)
        names = [n for n, _ in ev]
        k1 = names.index("ready")
        assert names[:k1 + 1] == ["tanh_bwd", "conv2d_bwd_filter", "conv2d_bwd_data", "modconv.dot", "gemm", "colsum", "ready"]
        _, wg, dg, ds2, gA, ga, rdy = [a for _, a in ev[:k1 + 1]]
        assert ev[k1][1] == net._train_range(s2)
        dz2, dxs = ctx.dz[2], ctx.dz[1]
        assert wg["x"] is ctx.mod_xs[2] and wg["dy"].data_ptr() == dz2.data_ptr() and (wg["beta"], wg["scale"]) == (0.5, 2.0)
        assert wg["dw"].data_ptr() == store.grad_of(rgb, "kernel").data_ptr()
        assert dg["epi"]["mode"] == ops.EPI_NONE and dg["epi"]["ref"] is None and dg["dx"].data_ptr() == dxs.data_ptr()       # unfused: ds needs it
        sc = ctx.mod_scratch(2)
        assert ds2["a"].data_ptr() == ctx.a[1].data_ptr() and ds2["b"].data_ptr() == dxs.data_ptr() and ds2["out"] is sc[2]
        assert (ds2["B"], ds2["P"], ds2["Cc"], ds2["beta"], ds2["scale"]) == (B, 64, 8, 0.0, 1.0)
        assert gA["A"].data_ptr() == z.data_ptr() and gA["Bm"] is sc[2] and gA["Cm"].data_ptr() == store.grad_of(rgb, "style_kernel").data_ptr()
        assert (gA["M"], gA["N"], gA["K"], gA["transA"], gA["beta"], gA["scale"]) == (Ls, 8, B, True, 0.5, 2.0)
        assert ga["x"] is sc[2] and ga["out"].data_ptr() == store.grad_of(rgb, "style_bias").data_ptr() and (ga["M"], ga["N"]) == (B, 8)
        rest = ev[k1 + 1:]
        rn = [n for n, _ in rest]
        k2 = rn.index("ready")
        assert rn[:k2 + 2] == ["modconv.scale", "mul_grad", "colsum", "modconv.dot", "modconv.scale", "conv2d_bwd_filter", "conv2d_fwd", "modconv.dot",
                               "modconv.demod_bwd", "modconv.scale", "gemm", "modconv.wsq_grad", "gemm", "colsum", "ready", "modconv.scale"]
        dx2, mg, cb, dd, dzs, wg1, dg1, ds1, db, sq, gq, wq, gA1, ga1, rdy1, dx1 = [a for _, a in rest[:k2 + 2]]
        assert rest[k2][1] == net._train_range(s1)
        assert dx2["x"].data_ptr() == dxs.data_ptr() == dx2["out"].data_ptr() and dx2["v"] is ctx.mod_s[2]              # dx = s * dxs, in place
        dz1 = ctx.dz[1]
        assert mg["ref"].data_ptr() == ctx.a[1].data_ptr() and mg["alpha"] == 0.2 and mg["out"].data_ptr() == dz1.data_ptr()
        assert cb["x"].data_ptr() == dz1.data_ptr() and cb["out"].data_ptr() == store.grad_of(t, "bias").data_ptr() and (cb["beta"], cb["scale"]) == (0.5, 2.0)
        s = ctx.mod_scratch(1)
        assert dd["a"].data_ptr() == dz1.data_ptr() and dd["b"] is ctx.z[1] and dd["out"] is s[0] and (dd["B"], dd["P"], dd["Cc"]) == (B, 64, 8)
        assert dzs["x"].data_ptr() == dz1.data_ptr() == dzs["out"].data_ptr() and dzs["v"] is ctx.mod_d[1] and dzs["bias"] is None
        assert wg1["dy"] is ctx.mod_xs[1] and wg1["x"].data_ptr() == dz1.data_ptr() and (wg1["beta"], wg1["scale"]) == (0.5, 2.0)     # a ConvT: sides swap
        assert dg1["x"].data_ptr() == dz1.data_ptr() and dg1["epi"]["mode"] == ops.EPI_NONE and dg1["y"].data_ptr() == ctx.dz[0].data_ptr()
        assert ds1["a"].data_ptr() == ctx.a[0].data_ptr() and ds1["b"].data_ptr() == ctx.dz[0].data_ptr() and ds1["out"] is s[2]
        assert db["d"] is ctx.mod_d[1] and db["dd"] is s[0] and db["s"] is ctx.mod_s[1] and db["q"] is store.mod_q(t) and db["dq"] is s[1] and db["ds"] is s[2]
        assert sq["x"] is ctx.mod_s[1] and sq["v"] is ctx.mod_s[1] and sq["out"] is s[3] and (sq["B"], sq["P"], sq["Cc"]) == (B, 1, 3)
        assert gq["A"] is s[3] and gq["Bm"] is s[1] and gq["Cm"] is s[4] and (gq["M"], gq["N"], gq["K"], gq["transA"]) == (3, 8, B, True)
        assert wq["w"] is t.vars["kernel"] and wq["dq"] is s[4] and wq["dw"].data_ptr() == store.grad_of(t, "kernel").data_ptr()
        assert (wq["taps"], wq["I"], wq["O"], wq["transposed"], wq["scale"]) == (9, 3, 8, True, 2.0)
        assert gA1["Cm"].data_ptr() == store.grad_of(t, "style_kernel").data_ptr() and ga1["out"].data_ptr() == store.grad_of(t, "style_bias").data_ptr()
        assert dx1["x"].data_ptr() == ctx.dz[0].data_ptr() == dx1["out"].data_ptr() and dx1["v"] is ctx.mod_s[1]
        assert rn[k2 + 2] == "pixelnorm.bwd"


def test_a_generator_without_the_layer_enqueues_none_of_it():
    maker.ensure_library(ROOT)
    for kw in (dict(), dict(normalization="pixel")):
        g = models.DCGANGenerator(arch="tiny", **kw)
        g.build("cpu")
        net = g.net()
        rec = _Recorder()
        with recording(rec):
            ctx = net.context(2, "test")
            net.forward(ctx, torch.zeros(2, 10), training=True)
            net.backward(ctx, torch.zeros(2, 8, 8, 3), need_dx=False, need_dw=True)
        assert not [n for n, _ in rec.events if n.startswith("modconv.")] and ctx.mod_w is None


# ------------------------------------------------------------------ 4. the reference itself
def _layer_case(kind, stride, seed, B=2, H=3, I=3, O=2, Ls=4, k=3):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    Wk = r(k, k, O, I) if kind == "convT" else r(k, k, I, O)
    return dict(x=r(B, H, H, I), w=r(B, Ls), Wk=Wk * 0.5, A=r(Ls, I) * 0.5, a=1.0 + 0.3 * r(I), bias=r(O) * 0.1), stride


@pytest.mark.parametrize("kind,stride", [("conv", 1), ("conv", 2), ("convT", 1), ("convT", 2)])
@pytest.mark.parametrize("demodulate", [True, False])
def test_unfused_form_equals_per_sample_modulated_weights(kind, stride, demodulate):
    c, stride = _layer_case(kind, stride, 7)
    a = MC.torch_modconv(kind, stride=stride, demodulate=demodulate, **c)
    b = MC.fused_modconv(kind, stride=stride, demodulate=demodulate, **c)
    assert a.shape == b.shape and float((a - b).abs().max()) < 1e-12 * max(1.0, float(b.abs().max()))
    assert float(b.abs().max()) > 0.1


@pytest.mark.parametrize("kind,stride", [("conv", 1), ("convT", 2)])
def test_written_out_backward_equals_autograd_and_autograd_equals_differences(kind, stride):
    """2 samples, 3x3 maps, I = 3, O = 2."""
    c, stride = _layer_case(kind, stride, 11)
    leaves = {n: t.clone().requires_grad_(True) for n, t in c.items()}
    y = MC.torch_modconv(kind, stride=stride, **leaves)
    dy = torch.randn(y.shape, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    want = torch.autograd.grad((y * dy).sum(), [leaves[n] for n in ("Wk", "bias", "A", "a", "x")])
    got = MC.manual_backward(kind, stride=stride, dy=dy, **c)
    for n, g, w in zip(("dW", "dbias", "dA", "da", "dx"), got, want):
        assert float((g - w).abs().max()) < 1e-11 * max(1.0, float(w.abs().max())), n
        assert float(w.abs().max()) > 1e-3, n
    f = lambda x, w, Wk, A, a, bias: MC.torch_modconv(kind, x, w, Wk, A, a, bias, stride)
    assert torch.autograd.gradcheck(f, [leaves[n] for n in ("x", "w", "Wk", "A", "a", "bias")], eps=1e-6, atol=1e-6, rtol=1e-5)


def test_walker_reads_the_style_source_behind_the_latent_normalisation():
    bg.set_seed(4)
    rng = np.random.default_rng(4)
    g = models.DCGANGenerator(arch="tiny_mnist", normalization="style", normalize_latents=True, noise=True, equalized_lr=True)
    g.build("cpu")
    MC.randomize(g, rng)
    import ln_reference as LN
    import pixelnorm_reference as PR
    W, train = LN.ref_params(g)
    z = torch.as_tensor(rng.uniform(size=(2, 6)))
    maps = rng.normal(size=(2, MC.noise_pixels(g)))
    with PR.walker(), MC.walker([maps, maps]) as qs:
        y = LN.ref_forward(g, W, z, True)
        y2 = LN.ref_forward(g, W, 3.0 * z, True)
    assert y.shape == (2, 12, 12, 1) and len(qs) == 4 and min(qs) > 0
    assert float((y - y2).detach().abs().max()) < 1e-6          # the latents' normalisation removes the scale everywhere: w and the Dense read it
    grads = torch.autograd.grad(y.sum(), train)
    assert all(float(g.abs().max()) > 0 for g in grads)
