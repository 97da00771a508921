"""layers.PixelNormalization without a GPU: the layer's surface, every placement rule of engine.Net, the generator variants of
models.py and the demos, what the case list of the kernel tests reaches according to bg_pixelnorm_route, what a generator with the
layer enqueues (and that one without it enqueues nothing new), the generated code of csrc/pixelnorm.hip, the formula pair against a
finite difference, and the argument errors of the C entry points."""
import contextlib
import ctypes as C
import importlib.util
import inspect
import os
import re

import numpy as np
import pytest
import torch

import blurred_gan_amd as bg
from blurred_gan_amd import _lib, layers, models, ops
import pixelnorm_cases as PC
import pixelnorm_reference as PR

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
L = layers

_spec = importlib.util.spec_from_file_location("make_engine_trace", os.path.join(HERE, "golden", "make_engine_trace.py"))
maker = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(maker)


# ------------------------------------------------------------------ 1. the layer
def test_layer_surface():
    l = L.PixelNormalization()
    assert (l.kind, l.epsilon) == ("pixelnorm", 1e-8)
    assert l.out_shape((4, 4, 32)) == (4, 4, 32) and l.out_shape((100,)) == (100,)
    assert l.var_specs((4, 4, 32)) == [] and l.count_params() == 0 and not l.vars
    assert L.PixelNormalization(epsilon=1e-4).epsilon == 1e-4
    for eps in (0, 0.0, -1e-8):
        with pytest.raises(ValueError, match="epsilon"):
            L.PixelNormalization(epsilon=eps)
    for shape in ((4, 32), (2, 4, 4, 32), ()):
        with pytest.raises(NotImplementedError, match=r"\[H, W, C\] map or a \[C\] vector"):
            l.out_shape(shape)


# ------------------------------------------------------------------ 2. placement
def _net(ls):
    m = L.Sequential(ls)
    m.build("cpu")
    return m.net()


def _refused(ls, match="PixelNormalization is supported directly behind the LeakyReLU"):
    with pytest.raises(NotImplementedError, match=match):
        _net(ls)


def test_placement_rules():
    PN, LR = L.PixelNormalization, L.LeakyReLU
    first = dict(input_shape=(4, 4, 3))
    conv = lambda **kw: L.Conv2D(8, 3, padding="same", **kw)
    convT = lambda **kw: L.Conv2DTranspose(8, 3, strides=2, padding="same", **kw)
    out = lambda: L.Conv2D(3, 3, padding="same", activation="tanh")
    # accepted: behind the LeakyReLU of a conv, a transposed conv, a Dense through its Reshape, a Dense itself; the latents
    net = _net([conv(**first), LR(), PN(), convT(), LR(0.2), PN(), out()])
    assert [st.kind for st in net.stages] == ["conv", "convT", "conv"]
    assert [st.pn is not None for st in net.stages] == [True, True, False] and [st.pn_channels for st in net.stages] == [8, 8, None]
    assert net.stages[1].alpha == 0.2 and net.has_pn and net.latent_pn is None
    assert [st.fusable_grad for st in net.stages] == [False, False, False]
    net = _net([L.Dense(48, input_shape=(5,)), L.Reshape((4, 4, 3)), LR(), PN(), conv(), LR(), out()])
    assert [st.kind for st in net.stages] == ["dense", "conv", "conv"] and net.stages[0].pn_channels == 3 and net.stages[0].pn_rows == 16
    assert net.stages[1].pn is None and net.stages[1].fusable_grad
    net = _net([L.Dense(48, input_shape=(5,)), LR(), PN(), L.Reshape((4, 4, 3)), out()])
    assert net.stages[0].pn_channels == 48 and net.stages[0].pn_rows == 1
    net = _net([PN(input_shape=(5,)), L.Dense(48, use_bias=False), L.BatchNormalization(), LR(), L.Reshape((4, 4, 3)), out()])
    assert net.latent_pn is not None and net.has_pn and [st.pn for st in net.stages] == [None, None] and net.in_shape == (5,)
    with pytest.raises(NotImplementedError, match="latents' normalisation has no backward"):
        net.backward(None, None, need_dx=True)
    # the existing refusal of a Dense + activation holds for a Dense stage without the layer
    _refused([L.Dense(48, input_shape=(5,)), LR(), L.Reshape((4, 4, 3)), out()], "Dense \\+ activation without BatchNormalization")
    # refused, with the rule in the message
    _refused([conv(**first), PN(), LR(), out()])                                            # before the activation
    _refused([conv(**first), LR(), PN(), PN(), out()])                                      # twice in a stage
    _refused([conv(**first), LR(), L.UpSampling2D(), PN(), out()])                          # behind a resampling layer
    _refused([conv(**first), LR(), L.AveragePooling2D(), PN(), out()])
    _refused([conv(**first), L.BatchNormalization(), LR(), PN(), out()])                    # with BatchNormalization
    _refused([conv(**first), L.LayerNormalization(), LR(), PN(), out()])                    # with LayerNormalization
    _refused([conv(**first), LR(), L.Dropout(0.3), PN(), out()])                            # with Dropout, either side
    _refused([conv(**first), LR(), PN(), L.Dropout(0.3), out()])
    _refused([conv(**first), LR(), PN(), L.BatchNormalization(), out()])
    _refused([conv(**first), LR(), PN(), LR(), out()])
    _refused([L.Conv2D(3, 3, padding="same", activation="tanh", **first), PN()])             # behind tanh
    _refused([L.Dense(48, input_shape=(5,)), LR(), L.Reshape((4, 4, 3)), PN(), out()])       # not directly behind the LeakyReLU
    _refused([PN(**first), conv(), LR(), out()])                                            # first, but on a map
    _refused([conv(**first), LR(), L.MinibatchStdDev(2), PN(), L.Flatten(), L.Dense(1)], "MinibatchStdDev is supported|PixelNormalization is supported")
    _refused([conv(**first), LR(), PN(), L.MinibatchStdDev(2), L.Flatten(), L.Dense(1)])    # a MinibatchStdDev behind the stage
    plain = _net([conv(**first), LR(), out()])
    assert not plain.has_pn and plain.stages[0].fusable_grad


def test_the_penalty_and_wgan_refuse_a_critic_with_the_layer():
    critic = lambda: L.Sequential([L.Conv2D(8, 3, strides=2, padding="same", input_shape=(8, 8, 3)), L.LeakyReLU(), L.PixelNormalization(),
                                   L.Flatten(), L.Dense(1)])
    m = critic()
    m.build("cpu")
    for call in (lambda n: n.gp_second_order(None, None), lambda n: n.gp_second_order_merged(None, 0, 2)):
        with pytest.raises(NotImplementedError, match="PixelNormalization in a critic under the gradient penalty is not built"):
            call(m.net())
    gen = models.DCGANGenerator(arch="tiny")
    gen.build("cpu")
    for cls in (bg.WGAN, bg.WGANGP):
        with pytest.raises(NotImplementedError, match="PixelNormalization in the discriminator"):
            cls(gen, m, cls.HyperParameters(batch_size=2, global_batch_size=2), bg.TrainingConfig(log_dir=os.devnull))


# ------------------------------------------------------------------ 3. models and demos
def _entries(m):
    m.build("cpu")
    own = {id(l) for l in m._own_layers()}
    return [(type(l).__name__, n, tuple(shape), tr) for (l, n, _, shape, tr) in m.store.entries if id(l) in own]


@pytest.mark.parametrize("up", ["transpose", "resize"])
@pytest.mark.parametrize("arch", sorted(models._G))
def test_generator_builder(arch, up):
    bg.set_seed(11)
    old = models.DCGANGenerator(arch=arch, upsampling=up)
    e_old, w_old = _entries(old), old.get_weights()
    bg.set_seed(11)
    batch = models.DCGANGenerator(arch=arch, upsampling=up, normalization="batch", normalize_latents=False)
    assert _entries(batch) == e_old and [l.kind for l, _ in batch.flat_layers()] == [l.kind for l, _ in old.flat_layers()]
    assert all(np.array_equal(a, b) for a, b in zip(batch.get_weights(), w_old))          # the same store, bit for bit
    assert (batch.normalization, batch.normalize_latents) == ("batch", False) == (old.normalization, old.normalize_latents)
    pix = models.DCGANGenerator(arch=arch, upsampling=up, normalization="pixel")
    kinds = [l.kind for l, _ in pix.flat_layers()]
    assert "bn" not in kinds and kinds[:4] == ["dense", "reshape", "lrelu", "pixelnorm"] and kinds[-1] in ("conv", "convT")
    hidden = [i for i, (l, _) in enumerate(pix.flat_layers()) if l.kind in ("dense", "conv", "convT")][:-1]
    assert kinds.count("pixelnorm") == len(hidden) == kinds.count("lrelu")
    base, ch, convt, last = models._G[arch]
    e = _entries(pix)
    assert [n for _, n, _, _ in e] == ["kernel", "bias"] * len(hidden) + ["kernel"] and all(tr for *_, tr in e)
    assert e[0][2] == (models.LATENT[arch], base * base * ch) and e[1][2] == (base * base * ch,)
    kernels_old = [sh for _, n, sh, _ in e_old if n == "kernel"]
    assert [sh for _, n, sh, _ in e if n == "kernel"] == kernels_old
    assert all(sh == (l.out_shape(s)[-1],) for (l, s) in pix.flat_layers() for n, sh, _, _ in l.var_specs(s) if n == "bias")
    assert pix.output_shape == (None,) + models.IMAGE_SHAPE[arch] == old.output_shape
    net = pix.net()
    assert [st.pn is not None for st in net.stages if st.kind not in ("upsample",)] == [True] * len(hidden) + [False]
    assert net.latent_pn is None and net.stages[0].pn_channels == ch and net.stages[0].pn_rows == base * base
    for norm in ("batch", "pixel"):
        lat = models.DCGANGenerator(arch=arch, upsampling=up, normalization=norm, normalize_latents=True)
        flat = lat.flat_layers()
        assert flat[0][0].kind == "pixelnorm" and flat[0][1] == (models.LATENT[arch],) and flat[1][0].kind == "dense"
        assert lat.input_shape == (None, models.LATENT[arch]) and lat.output_shape == old.output_shape
        assert len(_entries(lat)) == len(e if norm == "pixel" else e_old) and lat.net().latent_pn is flat[0][0]
    sn = models.DCGANGenerator(arch=arch, upsampling=up, normalization="pixel", spectral_norm=True)
    assert len(sn.net().spectral_layers) == len(hidden) + 1 and sum(st.pn is not None for st in sn.net().stages) == len(hidden)
    for bad in ("layer", None, "Pixel", True):
        with pytest.raises(ValueError, match="normalization must be 'batch' or 'pixel'"):
            models.DCGANGenerator(arch=arch, normalization=bad)


def test_models_docstring_names_the_keywords():
    assert 'normalization="pixel"' in models.__doc__ and "normalize_latents=True" in models.__doc__


def test_demos_take_the_switches():
    import demo_celeba
    import demo_mnist
    for demo in (demo_mnist, demo_celeba):
        args = demo.make_parser().parse_args([])
        assert args.generator_norm == "batch" and args.normalize_latents is False
        args = demo.make_parser().parse_args(["--generator-norm", "pixel", "--normalize-latents"])
        assert args.generator_norm == "pixel" and args.normalize_latents is True
        kinds = lambda m: [l.kind for l in m.layers]
        bg.set_seed(2)
        old = demo.DCGANGenerator()
        bg.set_seed(2)
        assert _entries(demo.DCGANGenerator(normalization="batch")) == _entries(old) and "pixelnorm" not in kinds(old)
        for up in ("transpose", "resize"):
            g = demo.DCGANGenerator(normalization="pixel", normalize_latents=True, upsampling=up)
            assert kinds(g)[:5] == ["pixelnorm", "dense", "reshape", "lrelu", "pixelnorm"] and "bn" not in kinds(g)
            g.build("cpu")
            assert g.net().latent_pn is not None and g.output_shape == old.output_shape


# ------------------------------------------------------------------ 4. what the case list reaches, from bg_pixelnorm_route alone
@pytest.fixture(scope="module")
def routes():
    maker.ensure_library(ROOT)
    return {(name, off): ops.pixelnorm.route(Cc, aligned=off == 0) for name, _, Cc, _ in PC.CASES for off in PC.OFFSETS}


def _family(r):
    return (r["vec"], "chunked" if r["chunks"] > 1 else r["regs"])


def test_case_list_reaches_every_route_and_its_first_and_last_c(routes):
    fam = {}
    for (name, off), r in routes.items():
        fam.setdefault(_family(r), set()).add(PC.case(name)[2])
    assert set(fam) == {(v, k) for v in (4, 1) for k in (1, 2, 4, "chunked")}, sorted(fam, key=str)
    # the first and the last C of each family, found by walking C itself (aligned views; a misaligned one takes the scalar families)
    span = {}
    for Cc in range(1, 2100):
        k = _family(ops.pixelnorm.route(Cc))
        lo, hi = span.get(k, (Cc, Cc))
        span[k] = (min(lo, Cc), max(hi, Cc))
    assert span[(4, 1)] == (4, 256) and span[(4, 2)] == (260, 512) and span[(4, 4)] == (516, 1024) and span[(4, "chunked")][0] == 1028
    assert span[(1, 1)] == (1, 63) and span[(1, 2)] == (65, 127) and span[(1, 4)] == (129, 255) and span[(1, "chunked")][0] == 257
    for k, (lo, hi) in span.items():
        assert lo in fam[k], (k, lo)
        assert k[1] == "chunked" or hi in fam[k], (k, hi)
    # lanes per row: every power of two, on either width; chunk counts: two or more with a ragged last chunk
    for vec in (4, 1):
        assert {r["lanes"] for r in routes.values() if r["vec"] == vec} == {1, 2, 4, 8, 16, 32, 64}, vec
    chunked = [(PC.case(n)[2], r) for (n, off), r in routes.items() if r["chunks"] > 1]
    assert any((Cc // r["vec"]) % 64 for Cc, r in chunked) and any((Cc // r["vec"]) % 64 == 0 for Cc, r in chunked)
    assert all(r["chunks"] == -(-(Cc // r["vec"]) // 64) for Cc, r in chunked)


def test_case_list_reaches_the_row_edges_and_every_alpha(routes):
    by_c = {}
    for name, R, Cc, alpha in PC.CASES:
        by_c.setdefault(Cc, set()).add(R)
    for Cc in (32, 4):
        rpw = ops.pixelnorm.route(Cc)["rows_per_workgroup"]
        assert {rpw - 1, rpw + 1} <= by_c[Cc], (Cc, rpw, sorted(by_c[Cc]))
    rpw = ops.pixelnorm.route(4)["rows_per_workgroup"]
    assert rpw == 256 and max(by_c[4]) > PC.MAX_BLOCKS * rpw and max(by_c[4]) * 4 * 4 < 8 << 20       # a second trip, a few MB
    assert 1 in by_c[32]
    for off in PC.OFFSETS:
        seen = {(PC.case(n)[3], r["chunks"] > 1) for (n, o), r in routes.items() if o == off}
        assert seen >= {(a, c) for a in (1.0, 0.2, 0.0) for c in (False, True)} | {(0.3, False)}, seen
    stock = {(R, Cc) for _, R, Cc, _ in PC.CASES}
    assert {(4, 100), (4, 10), (5, 6), (16, 32), (64, 16), (64, 512)} <= stock
    assert {Cc for _, _, Cc, _ in PC.CASES} >= {1, 3, 4, 5, 252, 256, 260, 512, 516, 1024, 1028, 257, 911}


def test_route_of_the_stock_shapes(routes):
    for Cc in (512, 256, 128, 64, 32, 16, 8, 4, 100, 10, 6):
        r = ops.pixelnorm.route(Cc)
        assert r["chunks"] == 1 and r["vec"] == (4 if Cc % 4 == 0 else 1) and r["lanes"] * r["regs"] * r["vec"] >= Cc, (Cc, r)
        assert r["rows_per_workgroup"] == 4 * 64 // r["lanes"]


# ------------------------------------------------------------------ 5. what a generator with the layer enqueues
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
    patch(bg.dist, "GradReducer", lambda *a, **k: rec)
    patch(layers, "default_device", lambda: torch.device("cpu"))
    try:
        yield rec
    finally:
        for obj, name, old in reversed(saved):
            setattr(obj, name, old)


def _cpu_gan(B=2, up="transpose", **gen_kw):
    bg.layers.set_seed(3)
    gen, disc = models.DCGANGenerator(arch="tiny", upsampling=up, **gen_kw), models.DCGANDiscriminator(arch="tiny")
    gen.build("cpu"), disc.build("cpu")
    hp = bg.WGANGP.HyperParameters(batch_size=B, global_batch_size=B)
    return bg.WGANGP(gen, disc, hp, bg.TrainingConfig(log_dir=os.devnull), step_replay=False)


@pytest.mark.parametrize("up", ["transpose", "resize"])
@pytest.mark.parametrize("latents", [False, True])
def test_launch_record_of_a_net_pass(up, latents):
    """Net.forward and Net.backward of a pixel-norm generator: per stage the linear op into z, then ONE forward launch; per stage ONE
    backward launch, in place in the stage's dz buffer; the latents' launch keeps no r; no BatchNormalization launch anywhere."""
    maker.ensure_library(ROOT)
    B = 2
    bg.layers.set_seed(3)
    gen = models.DCGANGenerator(arch="tiny", upsampling=up, normalization="pixel", normalize_latents=latents)
    gen.build("cpu")
    net = gen.net()
    pn = [i for i, st in enumerate(net.stages) if st.pn is not None]
    assert len(pn) == 4
    rec = _Recorder()
    with recording(rec):
        ctx = net.context(B, "test")
        for training in (False, True):          # the same launches in inference and in training
            del rec.events[:]
            net.forward(ctx, torch.zeros(B, 10), training=training)
            fwd_events = list(rec.events)
            names = [n for n, _ in fwd_events]
            assert names.count("pixelnorm.fwd") == len(pn) + latents and not [n for n in names if n.startswith("bn_")]
            calls = [a for n, a in fwd_events if n == "pixelnorm.fwd"]
            if latents:
                assert names.index("pixelnorm.fwd") < names.index("gemm") and calls[0]["r"] is None and calls[0]["lrelu_alpha"] == 1.0
                assert (calls[0]["R"], calls[0]["Cc"]) == (B, 10) and calls[0]["y"] is not calls[0]["x"]
                calls = calls[1:]
            for i, a in zip(pn, calls):
                st = net.stages[i]
                assert a["x"] is ctx.z[i] and a["y"] is ctx.a[i] and a["r"] is ctx.inv[i] and a["r"].numel() == B * st.pn_rows
                assert (a["R"], a["Cc"], a["eps"], a["lrelu_alpha"]) == (B * st.pn_rows, st.pn_channels, 1e-8, st.alpha)
                k = next(j for j, (_, args) in enumerate(fwd_events) if args is a)
                before = fwd_events[k - 1]
                assert before[0] == ("gemm" if st.kind == "dense" else "conv2d_bwd_data" if st.kind == "convT" else "conv2d_fwd")
                if st.kind == "dense":
                    assert before[1]["Cm"] is ctx.z[i] and before[1]["bias"] is not None
        del rec.events[:]
        net.backward(ctx, torch.zeros(B, 8, 8, 3), need_dx=False, need_dw=True)
        names = [n for n, _ in rec.events]
        bwd = [a for n, a in rec.events if n == "pixelnorm.bwd"]
        assert len(bwd) == len(pn) and "mul_grad" not in names and not [n for n in names if n.startswith("bn_")]
        for i, a in zip(reversed(pn), bwd):
            st = net.stages[i]
            assert a["g"].data_ptr() == a["dz"].data_ptr() == ctx.dz[i].data_ptr()         # in place: the route holds the row
            assert a["y"] is ctx.a[i] and a["r"] is ctx.inv[i] and (a["R"], a["Cc"], a["lrelu_alpha"]) == (B * st.pn_rows, st.pn_channels, st.alpha)
        # a bias gradient per pn stage, from dz, by the existing colsum
        assert names.count("colsum") == len(pn)
        if latents:
            with pytest.raises(NotImplementedError, match="no backward"):
                net.backward(ctx, torch.zeros(B, 8, 8, 3), need_dx=True)


def test_launch_record_of_a_training_step():
    maker.ensure_library(ROOT)
    rec = _Recorder()
    with recording(rec):
        gan = _cpu_gan(normalization="pixel", normalize_latents=True)
        gan.train_on_batch(np.zeros((2, 8, 8, 3), np.float32))
    names = [n for n, _ in rec.events]
    # D-step: the generator's inference forward; G-step: its training forward and backward
    assert names.count("pixelnorm.fwd") == 2 * (4 + 1) and names.count("pixelnorm.bwd") == 4
    assert not [n for n in names if n.startswith("bn_")]
    assert names.index("pixelnorm.bwd") > max(i for i, n in enumerate(names) if n == "pixelnorm.fwd")


def test_a_batch_generator_enqueues_none_of_it():
    maker.ensure_library(ROOT)
    rec = _Recorder()
    with recording(rec):
        gan = _cpu_gan()
        gan.train_on_batch(np.zeros((2, 8, 8, 3), np.float32))
    names = [n for n, _ in rec.events]
    assert not [n for n in names if n.startswith("pixelnorm.")] and [n for n in names if n.startswith("bn_")]
    G = gan.generator.net()
    assert not G.has_pn and all(st.pn is None for st in G.stages)
    assert all("pn_latents" not in c._extra for c in G._ctx.values())


# ------------------------------------------------------------------ 6. the formula pair
@pytest.mark.parametrize("R,Cc,alpha", [(3, 1, 0.2), (4, 5, 0.2), (2, 32, 1.0), (2, 100, 0.0), (3, 17, 0.3)])
def test_backward_equals_a_central_difference_of_the_forward(R, Cc, alpha):
    """float64, h = 1e-6 on data of size 1: truncation ~h^2, rounding ~1e-16 / h, so agreement to 1e-7 relative -- to the size of the
    terms r * g the derivative is made of (at C = 1 they cancel down to g * epsilon * r^3: the difference quotient's rounding does not
    shrink with them)."""
    eps, h = 1e-8, 1e-6
    x, g = PC.data(R, Cc, seed=R * 100 + Cc)
    y, r = PR.np_fwd(x, eps, alpha)
    dz = PR.np_bwd(g, y, r, alpha)
    fd = np.zeros_like(x)
    for i in range(R):
        for j in range(Cc):
            e = np.zeros_like(x)
            e[i, j] = h
            fd[i, j] = ((PR.np_fwd(x + e, eps, alpha)[0] - PR.np_fwd(x - e, eps, alpha)[0]) * g).sum() / (2 * h)
    scale = np.abs(r[:, None] * g).max()
    assert np.abs(dz - fd).max() <= 1e-7 * scale, (np.abs(dz - fd).max(), scale)
    # and autograd through the torch branch of the step reference
    xt = torch.as_tensor(x, dtype=torch.float64).requires_grad_(True)
    yt = PR.torch_pixelnorm(torch.nn.functional.leaky_relu(xt, alpha), eps)
    gt, = torch.autograd.grad((yt * torch.as_tensor(g)).sum(), xt)
    np.testing.assert_allclose(yt.detach().numpy(), y, rtol=1e-14, atol=0)
    np.testing.assert_allclose(gt.numpy(), dz, rtol=1e-11, atol=1e-13 * scale)


def test_zero_rows_case_is_exact_in_float32():
    x, g, y, r, dz = PC.zero_rows()
    y32, r32 = PR.np_fwd(x.astype(np.float32), PC.EPS, 0.25)
    assert np.array_equal(y32, y) and np.array_equal(r32, r) and np.array_equal(PR.np_bwd(g.astype(np.float32), y32, r32, 0.25), dz)
    assert (y == 0).sum() >= 6 and (np.signbit(x) & (x == 0)).any()


def test_case_data_is_exact_in_float32():
    for name, R, Cc, _ in PC.CASES[:12]:
        x, g = PC.data(R, Cc, 1)
        assert np.array_equal(x.astype(np.float32).astype(np.float64), x) and np.array_equal(g.astype(np.float32).astype(np.float64), g)
        assert (x != 0).all() and np.abs(x).max() <= 2


# ------------------------------------------------------------------ 7. the C entry points
def test_argument_errors_are_statuses():
    maker.ensure_library(ROOT)
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    q = C.c_void_p(p.value + 128)
    bad_shape, null, unsupported, misaligned = -1, -6, -3, -2
    fwd = lambda R, Cc, x=p, y=q, eps=1e-8: lib.bg_pixelnorm_fwd_f32(x, y, None, R, Cc, eps, 1.0, None)
    bwd = lambda R, Cc, g=p, y=q, dz=p: lib.bg_pixelnorm_bwd_f32(g, y, q, dz, R, Cc, 1.0, None)
    for call in (fwd, bwd):
        assert call(0, 4) == bad_shape and call(4, 0) == bad_shape and call(-1, 4) == bad_shape
        assert call(1, 4, None) == null and b"null pointer" in lib.bg_last_error()
        assert call(1, 4, C.c_void_p(p.value + 1)) == misaligned
    assert fwd(1, 4, eps=0.0) == bad_shape
    assert lib.bg_pixelnorm_bwd_f32(p, q, None, p, 1, 4, 1.0, None) == null
    assert fwd(1, 2048, y=p) == unsupported and bwd(1, 2048) == unsupported and b"register routes only" in lib.bg_last_error()
    assert bwd(1, 4, y=p) == unsupported and b"must not alias y" in lib.bg_last_error()
    out = (C.c_int * _lib.PIXELNORM_ROUTE_INTS)()
    assert lib.bg_pixelnorm_route(0, out) == bad_shape and lib.bg_pixelnorm_route(4, None) == null
    assert lib.bg_pixelnorm_route(512, out) == 0 and list(out) == [4, 64, 2, 1, 1, 64, 1, 8]
    with pytest.raises(ops.BgDeviceError):          # the wrappers refuse host tensors before anything is launched
        ops.pixelnorm.fwd(torch.zeros(2, 4), torch.zeros(2, 4), 2, 4)


# ------------------------------------------------------------------ 8. the code objects
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_kernels_use_no_private_memory_no_lds_and_move_float4(tmp_path):
    import subprocess
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = tmp_path / "pixelnorm.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-ffp-contract=off", "-w", "--cuda-device-only", "-S",
                    os.path.join(ROOT, "blurred-gan_amd", "csrc", "pixelnorm.hip"), "-o", str(out)], check=True)
    isa = out.read_text()
    kernels = list(re.finditer(r"\.name:\s+(\S*_kernel\S*)\n(.*?)\.wavefront_size", isa, flags=re.S))
    names = [m.group(1) for m in kernels]
    # two widths x (1, 2, 4 units per lane + the chunked route), forward and backward
    assert len(names) == 16 and sum("pn_fwd_kernel" in n for n in names) == 8 == sum("pn_bwd_kernel" in n for n in names), names
    for m in kernels:
        for key in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
            v = re.search(r"\." + key + r":\s+(\d+)", m.group(2))
            assert v and int(v.group(1)) == 0, (m.group(1), key)
        v = re.search(r"\.vgpr_count:\s+(\d+)", m.group(2))
        assert v and int(v.group(1)) <= 64, (m.group(1), v and v.group(1))            # eight waves per SIMD
    assert len(re.findall(r"\.amdhsa_group_segment_fixed_size 0\n", isa)) == 16 == len(re.findall(r"\.amdhsa_group_segment_fixed_size", isa))
    for name in names:
        body = re.search(r"^" + re.escape(name) + r":(.*?)^\.Lfunc_end", isa, flags=re.S | re.M).group(1)
        wide = "ILi4E" in name
        assert ("global_store_dwordx4" in body) == wide and ("global_load_dwordx4" in body) == wide, name
        assert "atomic" not in body and "ds_" not in body.replace("ds_bpermute", "").replace("ds_swizzle", ""), name
