"""layers.NoiseInjection, the normal draw and the latent distribution without a GPU: the statistics of the draw's float64
restatement (tests/noise_reference.py), the layer's surface, every placement rule of engine.Net, the generator keyword of models.py
and the demos' switches, what the case list of the kernel tests reaches according to bg_noise_route, what a generator with the layer
enqueues (and that one without it enqueues nothing new), and the argument errors of the C entry points."""
import contextlib
import ctypes as C
import importlib.util
import inspect
import os

import numpy as np
import pytest
import torch

import blurred_gan_amd as bg
from blurred_gan_amd import _lib, layers, models, ops
import noise_cases as NC
import noise_reference as NR

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
L = layers

_spec = importlib.util.spec_from_file_location("make_engine_trace", os.path.join(HERE, "golden", "make_engine_trace.py"))
maker = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(maker)


# ------------------------------------------------------------------ 1. the draw's restatement
@pytest.mark.parametrize("seed,offset", [(0x1234567, 77), (123, 0), (5, 2 ** 33), (99, 1000)])
def test_restatement_statistics(seed, offset):
    """5 standard errors at n = 2^20: mean 1 / sqrt(n), variance sqrt(2 / n), fourth moment sqrt(96 / n), correlation 1 / sqrt(n / 2)."""
    z = NR.np_normal(1 << 20, seed, offset)
    st = NR.statistics(z)
    print(seed, offset, st)
    NR.check_statistics(st)


def test_restatement_layout_and_edges():
    """Counter addressing (a draw at offset + k blocks is the tail of the draw at offset), the third counter word, the pairing of the
    words, the exact zero at u1 = 1 and the bound at u1 = 2^-24."""
    a, b = NR.np_normal(64, 9, 100), NR.np_normal(44, 9, 105)
    assert np.array_equal(a[20:], b)
    assert np.array_equal(NR.np_normal(37, 9, 100), a[:37])
    w = NR.philox4x32_10(np.array([100], np.uint64), 9, 2)
    assert not np.array_equal(w, NR.philox4x32_10(np.array([100], np.uint64), 9, 0))
    top = 0xFFFFFFFF
    z = NR.normal_from_words(np.array([[top, 0, 0, 1 << 30], [0, 1 << 31, top, 3 << 30]], np.uint64))
    assert z[0, 0] == 0.0 and z[0, 1] == 0.0                        # u1 = 1: r = 0
    r = np.sqrt(48 * np.log(2))
    np.testing.assert_allclose(z[0, 2:], [0.0, r], atol=1e-15)      # u1 = 2^-24, u2 = 1/4: (cos, sin)(pi / 2)
    np.testing.assert_allclose(z[1, :2], [-r, 0.0], atol=1e-15)     # u2 = 1/2
    assert z[1, 2] == 0.0 and z[1, 3] == 0.0 and r < NR.MAX_ABS


# ------------------------------------------------------------------ 2. the layer
def test_layer_surface():
    l = L.NoiseInjection()
    assert l.kind == "noise" and l.out_shape((4, 4, 32)) == (4, 4, 32)
    (name, shape, trainable, init), = l.var_specs((4, 4, 32))
    assert (name, shape, trainable) == ("noise_strength", (1,), True) and np.array_equal(init(None), np.zeros(1, np.float32))
    for shape in ((32,), (4, 32), (2, 4, 4, 32)):
        with pytest.raises(NotImplementedError, match=r"\[H, W, C\] map"):
            l.out_shape(shape)


# ------------------------------------------------------------------ 3. placement
def _net(ls):
    m = L.Sequential(ls)
    m.build("cpu")
    return m.net()


def _refused(ls, match="NoiseInjection is supported directly behind a Conv2D or Conv2DTranspose"):
    with pytest.raises(NotImplementedError, match=match):
        _net(ls)


def test_placement_rules():
    NI, PN, LR = L.NoiseInjection, L.PixelNormalization, L.LeakyReLU
    first = dict(input_shape=(4, 4, 3))
    conv = lambda **kw: L.Conv2D(8, 3, padding="same", **kw)
    convT = lambda **kw: L.Conv2DTranspose(8, 3, strides=2, padding="same", **kw)
    out = lambda: L.Conv2D(3, 3, padding="same", activation="tanh")
    # accepted: behind a conv or a transposed conv, wrapped or not, in front of the LeakyReLU, with or without PixelNormalization
    net = _net([conv(**first), NI(), LR(), PN(), convT(), NI(), LR(0.2), out()])
    assert [st.kind for st in net.stages] == ["conv", "convT", "conv"]
    assert [st.noise is not None for st in net.stages] == [True, True, False] and [st.pn is not None for st in net.stages] == [True, False, False]
    assert net.has_noise and net.noise_pixels == 16 + 64 and net.stages[1].alpha == 0.2 and net.stages[1].noise_pixels == 64
    assert [st.fusable_grad for st in net.stages] == [False, True, False]           # the stored output carries LeakyReLU's branch
    for wrap in (lambda l: L.SpectralNormalization(l), lambda l: L.EqualizedLearningRate(l)):
        net = _net([wrap(conv(**first)), NI(), LR(), out()])
        assert net.stages[0].noise is not None and net.stages[0].lin.kind == "conv"
    # the strength lies inside its stage's slice of the trainable buffer, which the reducer hands over with the stage
    m = L.Sequential([conv(**first), NI(), LR(), convT(), NI(), LR(), out()])
    m.build("cpu")
    net, st = m.net(), m.store
    for s in net.stages[:2]:
        lo, hi = net._train_range(s)
        (off,) = [o for (l, n, o, _, _) in st.entries if l is s.noise]
        assert lo <= off < off + 4 == hi and net._train_range(s)[0] == st.train_range(s.lin)[0]
    assert net._train_range(net.stages[0])[1] == net._train_range(net.stages[1])[0]
    # refused, with the rule in the message
    _refused([conv(**first), L.BatchNormalization(), NI(), LR(), out()])                    # with BatchNormalization, either side
    _refused([conv(**first), NI(), L.BatchNormalization(), LR(), out()])
    _refused([conv(**first), L.LayerNormalization(), NI(), LR(), out()])                    # with LayerNormalization, either side
    _refused([conv(**first), NI(), L.LayerNormalization(), LR(), out()])
    _refused([conv(**first), NI(), LR(), L.Dropout(0.3), out()])                            # with Dropout
    _refused([L.Conv2D(3, 3, padding="same", activation="tanh", **first), NI()])            # with tanh
    _refused([conv(**first), LR(), NI(), out()])                                            # behind the activation
    _refused([conv(**first), LR(), PN(), NI(), out()])
    _refused([conv(**first), NI(), NI(), LR(), out()])                                      # twice in a stage
    _refused([conv(**first), NI(), out()])                                                  # a stage without a LeakyReLU
    _refused([conv(**first), NI()])
    _refused([L.Dense(48, input_shape=(5,)), L.Reshape((4, 4, 3)), NI(), LR(), PN(), out()])     # behind a Dense
    _refused([conv(**first), LR(), L.UpSampling2D(), NI(), out()])                          # behind a resampling layer
    _refused([conv(**first), LR(), L.AveragePooling2D(), NI(), out()])
    _refused([conv(**first), LR(), L.FilteredUpSampling2D(), NI(), out()])
    with pytest.raises((NotImplementedError, RuntimeError)):                               # first in the network
        _net([NI(**first), conv(), LR(), out()])
    plain = _net([conv(**first), LR(), out()])
    assert not plain.has_noise and plain.noise_pixels == 0 and plain.stages[0].noise is None


def test_the_penalty_and_wgan_refuse_a_critic_with_the_layer():
    critic = lambda: L.Sequential([L.Conv2D(8, 3, strides=2, padding="same", input_shape=(8, 8, 3)), L.NoiseInjection(), L.LeakyReLU(),
                                   L.Flatten(), L.Dense(1)])
    m = critic()
    m.build("cpu")
    for call in (lambda n: n.gp_second_order(None, None), lambda n: n.gp_second_order_merged(None, 0, 2)):
        with pytest.raises(NotImplementedError, match="NoiseInjection in a critic under the gradient penalty is not built"):
            call(m.net())
    gen = models.DCGANGenerator(arch="tiny")
    gen.build("cpu")
    for cls in (bg.WGAN, bg.WGANGP):
        with pytest.raises(NotImplementedError, match="NoiseInjection in the discriminator"):
            cls(gen, m, cls.HyperParameters(batch_size=2, global_batch_size=2), bg.TrainingConfig(log_dir=os.devnull))


# ------------------------------------------------------------------ 4. models, WGAN keywords, demos
def _entries(m):
    m.build("cpu")
    own = {id(l) for l in m._own_layers()}
    return [(type(l).__name__, n, tuple(shape), tr) for (l, n, _, shape, tr) in m.store.entries if id(l) in own]


@pytest.mark.parametrize("up", ["transpose", "resize", "filtered"])
@pytest.mark.parametrize("arch", sorted(models._G))
def test_generator_builder(arch, up):
    bg.set_seed(11)
    old = models.DCGANGenerator(arch=arch, upsampling=up, normalization="pixel")
    e_old, w_old = _entries(old), old.get_weights()
    bg.set_seed(11)
    off = models.DCGANGenerator(arch=arch, upsampling=up, normalization="pixel", noise=False)
    assert _entries(off) == e_old and [l.kind for l, _ in off.flat_layers()] == [l.kind for l, _ in old.flat_layers()]
    assert all(np.array_equal(a, b) for a, b in zip(off.get_weights(), w_old)) and off.noise is False is old.noise
    bg.set_seed(11)
    g = models.DCGANGenerator(arch=arch, upsampling=up, normalization="pixel", noise=True)
    flat = g.flat_layers()
    kinds = [l.kind for l, _ in flat]
    hidden = [i for i, (l, _) in enumerate(flat) if l.kind in ("conv", "convT") and l.activation is None]
    assert kinds.count("noise") == len(hidden) == len(models._G[arch][2]) - (models._G[arch][3] is None) and g.noise is True
    for i in hidden:        # conv -> NoiseInjection -> LeakyReLU -> PixelNormalization
        assert kinds[i + 1:i + 4] == ["noise", "lrelu", "pixelnorm"]
    e = _entries(g)
    assert [x for x in e if x[1] != "noise_strength"] == e_old
    assert [x for x in e if x[1] == "noise_strength"] == [("NoiseInjection", "noise_strength", (1,), True)] * len(hidden)
    ws = dict(zip([(i, x[1]) for i, x in enumerate(e)], g.get_weights()))
    assert all(np.array_equal(w, np.zeros(1)) for (i, n), w in ws.items() if n == "noise_strength")          # initialised to zeros
    net = g.net()
    assert net.has_noise and net.noise_pixels == sum(int(np.prod(flat[i][0].out_shape(flat[i][1])[:2])) for i in hidden)
    assert g.store.n_train == old.store.n_train + 4 * len(hidden)        # n_train separates the two models (the step key)
    assert g.output_shape == old.output_shape
    for kw in (dict(), dict(normalization="batch")):
        with pytest.raises(ValueError, match="noise=True needs normalization='pixel'"):
            models.DCGANGenerator(arch=arch, noise=True, **kw)


def test_celeba64_noise_maps():
    g = models.DCGANGenerator(arch="celeba64", normalization="pixel", noise=True, equalized_lr=True)
    g.build("cpu")
    net = g.net()
    assert [st.noise_pixels for st in net.stages if st.noise is not None] == [16, 64, 256, 1024, 4096] and net.noise_pixels == 5456
    assert len(net.eqlr_layers) == 7


def test_models_docstring_names_the_keyword():
    assert "``noise=True``" in models.__doc__ and "NoiseInjection" in models.__doc__


def _cpu_gan(B=2, cls=None, **kw):
    bg.layers.set_seed(3)
    gen_kw = kw.pop("gen_kw", dict(normalization="pixel", noise=True))
    gen, disc = models.DCGANGenerator(arch="tiny", **gen_kw), models.DCGANDiscriminator(arch="tiny")
    gen.build("cpu"), disc.build("cpu")
    cls = cls or bg.WGANGP
    return cls(gen, disc, cls.HyperParameters(batch_size=B, global_batch_size=B), bg.TrainingConfig(log_dir=os.devnull), step_replay=False, **kw)


def test_wgan_keywords():
    for bad in ("gaussian", None, "Normal", 1):
        with pytest.raises(ValueError, match="latent_distribution must be 'uniform' or 'normal'"):
            _cpu_gan(latent_distribution=bad)
    assert _cpu_gan().latent_distribution == "uniform" and _cpu_gan(latent_distribution="normal").latent_distribution == "normal"
    plain = _cpu_gan(gen_kw={})
    for key in ("noise_d", "noise_g"):
        with pytest.raises(ValueError, match="noise_d / noise_g"):
            plain.train_on_batch(np.zeros((2, 8, 8, 3), np.float32), randomness={key: np.zeros((2, 84), np.float32)})
    # the generator's seed: its own, per rank, not the critic's or the model stream's
    gan = _cpu_gan()
    assert gan._noise_seed() == gan._rng_seed + 15485863 and "rank" in inspect.getdoc(bg.WGAN._noise_seed)
    assert gan._noise_seed() not in (gan._rng_seed + 104729, gan._rng_seed)
    # the step key: the latents' distribution is part of it; the noise needs no field (n_train separates the models)
    reals = torch.zeros(2, 8, 8, 3)
    for m in (gan.generator, gan.discriminator):
        bg.optimizers.get_optimizer(m).attach(m.store)
    k_uniform = gan._step_key("d", reals)
    gan.latent_distribution = "normal"
    assert gan._step_key("d", reals) != k_uniform and "normal" in gan._step_key("g", reals)
    for m in (plain.generator, plain.discriminator):
        bg.optimizers.get_optimizer(m).attach(m.store)
    kp, kn = plain._step_key("g", reals), k_uniform
    assert plain.generator.store.n_train != gan.generator.store.n_train and plain.generator.store.n_train in kp
    assert gan.generator.store.n_train in kn


def test_demos_take_the_switches():
    import demo_celeba
    import demo_mnist
    for demo in (demo_mnist, demo_celeba):
        args = demo.make_parser().parse_args([])
        assert args.generator_noise is False and args.latent_distribution == "uniform"
        args = demo.make_parser().parse_args(["--generator-norm", "pixel", "--generator-noise", "--latent-distribution", "normal"])
        assert args.generator_noise is True and args.latent_distribution == "normal" and args.generator_norm == "pixel"
        with pytest.raises(SystemExit):
            demo.make_parser().parse_args(["--latent-distribution", "cauchy"])
        kinds = lambda m: [l.kind for l in m.layers]
        bg.set_seed(2)
        old = demo.DCGANGenerator(normalization="pixel")
        bg.set_seed(2)
        assert _entries(demo.DCGANGenerator(normalization="pixel", noise=False)) == _entries(old) and "noise" not in kinds(old)
        with pytest.raises(ValueError, match="noise=True needs normalization='pixel'"):
            demo.DCGANGenerator(noise=True)
        for up in ("transpose", "resize"):
            g = demo.DCGANGenerator(normalization="pixel", noise=True, upsampling=up)
            k = kinds(g)
            hidden = [i for i, l in enumerate(g.layers) if l.kind in ("conv", "convT") and l.activation is None]
            assert k.count("noise") == len(hidden) and all(k[i + 1:i + 4] == ["noise", "lrelu", "pixelnorm"] for i in hidden)
            g.build("cpu")
            assert g.net().has_noise and g.output_shape == old.output_shape


# ------------------------------------------------------------------ 5. what the case list reaches, from bg_noise_route alone
@pytest.fixture(scope="module")
def routes():
    maker.ensure_library(ROOT)
    return {(name, off): ops.noise.route(Cc, aligned=off == 0) for name, _, Cc in NC.CASES for off in NC.OFFSETS}


def _family(r):
    return (r["vec"], "chunked" if r["chunks"] > 1 else r["regs"])


def test_case_list_reaches_every_route_and_row_edge(routes):
    fam = {}
    for (name, off), r in routes.items():
        fam.setdefault(_family(r), set()).add(NC.case(name)[2])
    assert set(fam) == {(v, k) for v in (4, 1) for k in (1, 2, 4, "chunked")}, sorted(fam, key=str)
    assert {1, 3, 4, 8, 64} <= fam[(1, 1)] and {4, 8, 64} <= fam[(4, 1)]
    assert ops.noise.route(512) == ops.pixelnorm.route(512) and ops.noise.route(6, aligned=False) == ops.pixelnorm.route(6, aligned=False)
    chunked = [(NC.case(n)[2], r) for (n, off), r in routes.items() if r["chunks"] > 1]
    assert any((Cc // r["vec"]) % 64 for Cc, r in chunked) and any((Cc // r["vec"]) % 64 == 0 for Cc, r in chunked)
    by_c = {}
    for name, R, Cc in NC.CASES:
        by_c.setdefault(Cc, set()).add(R)
    for Cc in (1, 3, 4, 8, 64):
        assert {1, 7} <= by_c[Cc] and ops.noise.route(Cc)["rows_per_workgroup"] + 1 in by_c[Cc], (Cc, sorted(by_c[Cc]))
    assert ops.noise.route(4, aligned=False)["rows_per_workgroup"] + 1 in by_c[4]
    rpw = ops.noise.route(4)["rows_per_workgroup"]
    assert rpw == 256 and max(by_c[4]) > NC.MAX_BLOCKS * rpw and max(by_c[4]) * 4 * 4 < 8 << 20           # a second trip, a few MB
    # the gradient's workspace: one float per workgroup of the larger of a C's two grids
    for name, R, Cc in NC.CASES:
        need = max(min(-(-R // r["rows_per_workgroup"]), NC.MAX_BLOCKS) * r["chunks"] for r in (ops.noise.route(Cc), ops.noise.route(Cc, False)))
        assert ops.noise.workspace_bytes(R, Cc) == 4 * need, name


# ------------------------------------------------------------------ 6. what a generator with the layer enqueues
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
            if "counter" in args:
                args["counter_of"] = args["counter"]
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
    for name, ret in {"fwd": "y", "bwd": "dz"}.items():
        patch(ops.pixelnorm, name, staticmethod(rec.wrap(f"pixelnorm.{name}", getattr(ops.pixelnorm, name), ret)))
    for name, ret in {"add": "y", "grad": "dstrength"}.items():
        patch(ops.noise, name, staticmethod(rec.wrap(f"noise.{name}", getattr(ops.noise, name), ret)))
    patch(ops.rng, "normal", staticmethod(rec.wrap("rng.normal", ops.rng.normal, "out")))
    sig = inspect.signature(ops.epilogue)

    def epilogue(*a, **k):      # the descriptor as the keywords it was made from
        b = sig.bind(*a, **k)
        b.apply_defaults()
        return dict(b.arguments)
    patch(ops, "epilogue", epilogue)
    patch(ops, "conv2d_stats_rows", lambda epi: 0)
    patch(bg.dist, "GradReducer", lambda *a, **k: rec)
    patch(layers, "default_device", lambda: torch.device("cpu"))
    try:
        yield rec
    finally:
        for obj, name, old in reversed(saved):
            setattr(obj, name, old)


def _hand_built():
    bg.layers.set_seed(3)
    gen = NR.hand_built_generator("tiny")
    gen.build("cpu")
    return gen


@pytest.mark.parametrize("which", ["pixel", "resize", "hand_built"])
def test_launch_record_of_a_net_pass(which):
    """Net.forward and Net.backward of a generator with the layer: ONE normal draw per pass, over the one flat buffer, from the pass's
    seed and the network's counter; per noise stage ONE add, in place on what the conv (EPI_NONE + bias) wrote, in front of the
    PixelNormalization pass or with the stage's alpha; per noise stage ONE gradient launch sequence on the stage's dz, ahead of the
    hand-over of the stage's slice."""
    maker.ensure_library(ROOT)
    B = 2
    bg.layers.set_seed(3)
    if which == "hand_built":
        gen = _hand_built()
    else:
        gen = models.DCGANGenerator(arch="tiny", normalization="pixel", noise=True, upsampling="resize" if which == "resize" else "transpose")
        gen.build("cpu")
    net = gen.net()
    ns = [i for i, st in enumerate(net.stages) if st.noise is not None]
    assert len(ns) == 3 and net.noise_pixels == 4 + 16 + 64
    rec = _Recorder()
    with recording(rec):
        ctx = net.context(B, "test")
        assert ctx.noise_flat.numel() == B * net.noise_pixels
        o = 0
        for i in ns:        # stage by stage, each slice contiguous
            n = B * net.stages[i].noise_pixels
            assert ctx.noise[i].data_ptr() == ctx.noise_flat.data_ptr() + 4 * o and ctx.noise[i].numel() == n
            o += n
        for training in (False, True):          # the same launches in inference and in training
            del rec.events[:]
            off0 = net.rng_offset
            net.forward(ctx, torch.zeros(B, 10), training=training, seed=41)
            ev = list(rec.events)
            names = [n for n, _ in ev]
            assert names.count("rng.normal") == 1 and names.count("noise.add") == len(ns) and "uniform" not in names
            d = ev[names.index("rng.normal")][1]
            assert d["out"] is ctx.noise_flat and d["seed"] == 41 and d["offset"] == off0 and d["counter_of"] == (net, "rng_offset")
            assert net.rng_offset == off0 + (B * net.noise_pixels + 3) // 4
            assert names.index("rng.normal") < min(i for i, n in enumerate(names) if n.startswith("conv2d"))
            for i, (k, a) in zip(ns, [(k, a) for k, (n, a) in enumerate(ev) if n == "noise.add"]):
                st = net.stages[i]
                tgt = ctx.z[i] if st.pn is not None else ctx.a[i]
                assert a["x"] is tgt and a["y"] is tgt and a["noise"] is ctx.noise[i] and a["strength"] is st.noise.vars["noise_strength"]
                assert (a["R"], a["Cc"], a["lrelu_alpha"]) == (B * st.noise_pixels, st.out_shape[-1], 1.0 if st.pn is not None else st.alpha)
                before = ev[k - 1]
                assert before[0] == ("conv2d_bwd_data" if st.kind == "convT" else "conv2d_fwd")
                assert before[1]["epi"]["mode"] == ops.EPI_NONE and before[1]["epi"]["bias"] is st.lin.vars["bias"]
                assert before[1]["dx" if st.kind == "convT" else "y"] is tgt
                if st.pn is not None:
                    assert ev[k + 1][0] == "pixelnorm.fwd" and ev[k + 1][1]["x"] is tgt
        del rec.events[:]
        net.backward(ctx, torch.zeros(B, 8, 8, 3), need_dx=False, need_dw=True, beta=0.5, scale=2.0, reducer=rec)
        ev = list(rec.events)
        grads = [(k, a) for k, (n, a) in enumerate(ev) if n == "noise.grad"]
        assert len(grads) == len(ns)
        for i, (k, a) in zip(reversed(ns), grads):
            st = net.stages[i]
            assert a["dz"].data_ptr() == ctx.dz[i].data_ptr() and a["noise"].data_ptr() == ctx.noise[i].data_ptr()
            assert a["dstrength"].data_ptr() == gen.store.grad_of(st.noise, "noise_strength").data_ptr()
            assert (a["R"], a["Cc"], a["beta"], a["scale"]) == (B * st.noise_pixels, st.out_shape[-1], 0.5, 2.0)
            ready = next(j for j, (n, r) in enumerate(ev) if n == "ready" and r == net._train_range(st))
            assert k < ready
        # noise=False: neither a draw nor an add; the strengths' gradients are beta * old by a plain launch; a tensor: copied in
        del rec.events[:]
        net.forward(ctx, torch.zeros(B, 10), noise=False)
        names = [n for n, _ in rec.events]
        assert "rng.normal" not in names and "noise.add" not in names and not ctx.noise_active
        net.backward(ctx, torch.zeros(B, 8, 8, 3), need_dx=False, need_dw=True)
        assert "noise.grad" not in [n for n, _ in rec.events]
        del rec.events[:]
        maps = torch.arange(B * net.noise_pixels, dtype=torch.float32).view(B, net.noise_pixels)
        net.forward(ctx, torch.zeros(B, 10), noise=maps)
        names = [n for n, _ in rec.events]
        assert "rng.normal" not in names and names.count("noise.add") == len(ns) and ctx.noise_active
        o = 0
        for i in ns:        # [B, P] per sample in network order -> the stage's [B, H * W]
            n = net.stages[i].noise_pixels
            assert torch.equal(ctx.noise[i].view(B, n), maps[:, o:o + n])
            o += n
        with pytest.raises(ValueError, match="noise must be"):
            net.forward(ctx, torch.zeros(B, 10), noise=maps[:, :-1])


@pytest.mark.parametrize("latents", ["uniform", "normal"])
def test_launch_record_of_a_training_step(latents):
    maker.ensure_library(ROOT)
    rec = _Recorder()
    with recording(rec):
        gan = _cpu_gan(latent_distribution=latents)
        gan.train_on_batch(np.zeros((2, 8, 8, 3), np.float32))
        assert gan.latents_batch().shape == (2, 10)
    G = gan.generator.net()
    names = [n for n, _ in rec.events]
    draws = [a for n, a in rec.events if n == "rng.normal"]
    noise = [a for a in draws if a["counter_of"][1] == "rng_offset"]
    # D-step: the generator's inference forward; G-step: its training forward and backward
    assert len(noise) == 2 and all(a["counter_of"][0] is G and a["seed"] == gan._noise_seed() for a in noise)
    assert noise[0]["offset"] == 0 and noise[1]["offset"] == (2 * G.noise_pixels + 3) // 4          # successive steps see other noise
    assert names.count("noise.add") == 2 * 3 and names.count("noise.grad") == 3
    z = [a for a in draws if a["counter_of"] == (gan, "_rng_off")]
    uz = [a for n, a in rec.events if n == "uniform" and tuple(a["out"].shape) == (2, 10)]
    if latents == "normal":     # z_d, z_g and latents_batch(): the model's stream and counter, another kernel
        assert len(z) == 3 and not uz and all(a["seed"] == gan._rng_seed and tuple(a["out"].shape) == (2, 10) for a in z)
    else:
        assert not z and len(uz) == 3


def test_a_generator_without_the_layer_enqueues_none_of_it():
    maker.ensure_library(ROOT)
    for gen_kw in ({}, dict(normalization="pixel")):
        rec = _Recorder()
        with recording(rec):
            gan = _cpu_gan(gen_kw=gen_kw)
            gan.train_on_batch(np.zeros((2, 8, 8, 3), np.float32))
            gan.generate_samples()
        names = [n for n, _ in rec.events]
        assert not [n for n in names if n.startswith("noise.") or n.startswith("rng.")]
        G = gan.generator.net()
        assert not G.has_noise and all(c.noise_flat is None for c in G._ctx.values()) and G.rng_offset == 0


# ------------------------------------------------------------------ 7. the C entry points
def test_argument_errors_are_statuses():
    maker.ensure_library(ROOT)
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    q = C.c_void_p(p.value + 128)
    bad_shape, null, misaligned = -1, -6, -2
    add = lambda R, Cc, x=p, n=q, s=q, y=p: lib.bg_noise_add_f32(x, n, s, y, R, Cc, 1.0, None)
    grad = lambda R, Cc, dz=p, n=q, d=q, ws=q: lib.bg_noise_grad_f32(dz, n, d, R, Cc, ws, 0.0, 1.0, None)
    for call in (add, grad):
        assert call(0, 4) == bad_shape and call(4, 0) == bad_shape and call(-1, 4) == bad_shape
        assert call(1, 4, None) == null and b"null pointer" in lib.bg_last_error()
        assert call(1, 4, p, None) == null and call(1, 4, p, q, None) == null and call(1, 4, p, q, q, None) == null
        assert call(1, 4, C.c_void_p(p.value + 1)) == misaligned
    assert lib.bg_normal_f32(None, 4, 1, 0, None) == null and lib.bg_normal_f32(p, 0, 1, 0, None) == bad_shape
    assert lib.bg_normal_f32(C.c_void_p(p.value + 2), 4, 1, 0, None) == misaligned
    out = (C.c_int * _lib.NOISE_ROUTE_INTS)()
    assert lib.bg_noise_route(0, out) == bad_shape and lib.bg_noise_route(4, None) == null
    assert lib.bg_noise_route(512, out) == 0 and list(out) == [4, 64, 2, 1, 1, 64, 1, 8]
    assert lib.bg_noise_grad_workspace_bytes(0, 4) == 0 and lib.bg_noise_grad_workspace_bytes(7, 4) == 4
    with pytest.raises(ops.BgDeviceError):          # the wrappers refuse host tensors before anything is launched
        ops.noise.add(torch.zeros(2, 4), torch.zeros(2), torch.zeros(1), torch.zeros(2, 4), 2, 4)
    with pytest.raises(ops.BgDeviceError):
        ops.rng.normal(torch.zeros(8), 1)
