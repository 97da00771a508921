"""The FIR-filtered resampling layers without a GPU (layers.FilteredUpSampling2D / FilteredDownSampling2D): the layers' surface,
engine.Net's placement rules for the two new kinds, the "filtered" variants of the DCGAN stacks and of the demos, the reference
operators themselves (tests/firsample_reference.py against StyleGAN2's upfirdn restated, nearest / average pooling, bilinear
interpolation, the adjoint identity), what a filtered critic and a filtered generator enqueue, and the argument checks of
bg_fir_upsample2x_nhwc_f32 / bg_fir_downsample2x_nhwc_f32 (no device work is launched)."""
import contextlib
import importlib.util
import inspect
import os

import numpy as np
import pytest
import torch

import blurred_gan_amd as bg
from blurred_gan_amd import ema, layers, models, ops
from blurred_gan_amd.engine import Net
import firsample_reference as FR

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ARCHS = sorted(models.IMAGE_SHAPE)
UP, DOWN = layers.FilteredUpSampling2D, layers.FilteredDownSampling2D
ASYM = (1, 3, 2, 2)

_spec = importlib.util.spec_from_file_location("make_engine_trace", os.path.join(HERE, "golden", "make_engine_trace.py"))
maker = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(maker)


# ------------------------------------------------------------------ 1. layers
def test_shape_arithmetic():
    up, down = UP(), DOWN()
    assert (up.kind, down.kind) == ("firup", "firdown")
    assert up.out_shape((3, 5, 7)) == (6, 10, 7) and up.out_shape((1, 1, 1)) == (2, 2, 1)
    assert down.out_shape((6, 10, 7)) == (3, 5, 7) and down.out_shape((2, 2, 1)) == (1, 1, 1)
    assert down.out_shape(up.out_shape((4, 9, 2))) == (4, 9, 2)
    for l in (up, down):
        assert l.var_specs((4, 4, 8)) == [] and l.vars == {} and l.count_params() == 0


@pytest.mark.parametrize("kernel", [(1, 1), (1, 3, 3, 1), [1, 3, 2, 2], (1, 2, 5, 3), (1, 5, 10, 10, 5, 1), (1, 2, 3, 4, 2, 2, 1, 1),
                                    (0.5, 1.5), (-1, 9, 9, -1), np.array([1.0, 3.0, 3.0, 1.0])])
def test_taps_are_the_kernel_normalised_in_double_and_rounded_once(kernel):
    k = np.asarray(kernel, np.float64)
    want = (k / k.sum()).astype(np.float32)
    for cls in (UP, DOWN):
        l = cls(kernel)
        assert isinstance(l.taps, tuple) and all(type(t) is float for t in l.taps)
        assert np.array_equal(np.asarray(l.taps, np.float32), want) and np.array_equal(np.float32(l.taps), np.float64(l.taps))
        assert l.flipped_taps == l.taps[::-1] and l.resample_kernel == tuple(float(v) for v in kernel)
    assert FR.normalized(kernel) == UP(kernel).taps


def test_accepted_arguments():
    assert UP().taps == DOWN().taps == (0.125, 0.375, 0.375, 0.125)
    UP((1, 3, 3, 1), 2, None)
    UP(size=(2, 2), data_format="channels_last")
    DOWN((1, 1), 2, "channels_last")
    DOWN(factor=(2, 2))
    assert UP(ASYM).taps != UP(ASYM).flipped_taps            # asymmetric kernels are allowed


@pytest.mark.parametrize("cls", [UP, DOWN])
def test_argument_refusals(cls):
    for bad in ((1, float("nan")), (1, float("inf")), (1, -1), (0, 0), (-1, -3, -3, -1), "abcd", (1, "x"), 3, None, (), ((1, 2), (3, 4))):
        with pytest.raises(ValueError, match="resample_kernel"):
            cls(bad)
    for odd in ((1,), (1, 2, 1), (1, 4, 6, 4, 1), (1,) * 10, (1,) * 9):
        with pytest.raises(NotImplementedError, match="even lengths up to 8"):
            cls(odd)
    for factor in (1, 3, 4, (2, 1), (4, 4)):
        with pytest.raises(NotImplementedError, match="factor of 2"):
            cls((1, 3, 3, 1), factor)
    with pytest.raises(NotImplementedError, match="channels_last"):
        cls(data_format="channels_first")
    for shape in ((4, 8), (2, 4, 4, 8), (8,)):
        with pytest.raises(NotImplementedError, match=r"\[H, W, C\] map"):
            cls().out_shape(shape)


@pytest.mark.parametrize("shape", [(5, 4, 2), (4, 7, 2), (3, 3, 1)])
def test_downsampling_an_odd_map_is_refused_when_shapes_are_inferred(shape):
    with pytest.raises(NotImplementedError, match="odd"):
        DOWN().out_shape(shape)
    with pytest.raises(NotImplementedError, match="odd"):
        layers.Sequential([layers.Conv2D(4, 3, padding="same", input_shape=list(shape)), DOWN()])


def test_the_nearest_layers_still_refuse_bilinear():
    with pytest.raises(NotImplementedError):
        layers.UpSampling2D(interpolation="bilinear")
    with pytest.raises(ValueError):
        models.DCGANGenerator(arch="tiny", upsampling="bilinear")


# ------------------------------------------------------------------ 2. placement (engine.Net.__init__)
def _net(ls):
    m = layers.Sequential(ls)
    m.build("cpu")
    return Net(m.flat_layers(), m.store)


def _conv(**kw):
    return layers.Conv2D(4, 3, padding="same", **kw)


@pytest.mark.parametrize("resample", [UP, DOWN])
def test_placement_refusals(resample):
    with pytest.raises(NotImplementedError, match="first or last"):            # first stage
        _net([resample(input_shape=(4, 4, 2)), _conv()])
    with pytest.raises(NotImplementedError, match="first or last"):            # last stage
        _net([_conv(input_shape=(4, 4, 2)), resample()])
    with pytest.raises(NotImplementedError, match="first or last"):            # last stage behind views only
        _net([_conv(input_shape=(4, 4, 2)), resample(), layers.Flatten()])
    with pytest.raises(NotImplementedError, match="must directly follow a linear layer"):
        _net([_conv(input_shape=(4, 4, 2)), resample(), layers.BatchNormalization(), _conv()])
    with pytest.raises(NotImplementedError, match="must follow a linear layer"):
        _net([_conv(input_shape=(4, 4, 2)), resample(), layers.LeakyReLU(), _conv()])
    with pytest.raises(NotImplementedError, match="Dropout is supported after conv"):
        _net([_conv(input_shape=(4, 4, 2)), resample(), layers.Dropout(0.3), _conv()])
    with pytest.raises(NotImplementedError, match="LayerNormalization must directly follow a Conv2D"):
        _net([_conv(input_shape=(4, 4, 2)), resample(), layers.LayerNormalization(), layers.LeakyReLU(), _conv()])


def test_allowed_placements_compile_into_stages_of_their_own():
    net = _net([_conv(input_shape=(4, 4, 2)), layers.LeakyReLU(), layers.Dropout(0.3), DOWN(), UP(), _conv(), layers.BatchNormalization(),
                layers.LeakyReLU(), UP(ASYM), DOWN(ASYM), layers.AveragePooling2D(), layers.UpSampling2D(), layers.Flatten(), layers.Dense(1)])
    assert [st.kind for st in net.stages] == ["conv", "firdown", "firup", "conv", "firup", "firdown", "avgpool", "upsample", "dense"]
    assert [st.out_shape for st in net.stages] == [(4, 4, 4), (2, 2, 4), (4, 4, 4), (4, 4, 4), (8, 8, 4), (4, 4, 4), (2, 2, 4), (4, 4, 4), (1,)]
    assert len(net.conv_layers) == 2
    for st in net.stages:
        if st.kind in ("firup", "firdown"):
            assert st.bn is None and st.act is None and not st.drop and not st.fusable_grad
            assert net.store.train_range(st.lin, st.bn) == (0, 0)
    assert net.stages[0].fusable_grad            # the down-sampling stage's backward lands as this stage's dz
    ctx = net.context(3)
    assert ctx.keep[1] is None and ctx.z[1] is None and tuple(ctx.a[1].shape) == (3, 2, 2, 4)


def test_minibatch_stddev_stands_behind_a_filtered_downsampling():
    head = lambda: [layers.MinibatchStdDev(group_size=2), layers.Flatten(), layers.Dense(1)]
    net = _net([_conv(input_shape=(4, 4, 2)), layers.LeakyReLU(), DOWN()] + head())
    assert [st.kind for st in net.stages] == ["conv", "firdown", "mbstd", "dense"]
    with pytest.raises(NotImplementedError, match="MinibatchStdDev is supported directly before"):
        _net([_conv(input_shape=(4, 4, 2)), layers.LeakyReLU(), UP()] + head())


def test_the_penalty_takes_the_filtered_kinds_as_resampling_stages():
    net = _net([_conv(input_shape=(4, 4, 2)), layers.LeakyReLU(), DOWN(), UP(), _conv(), layers.LeakyReLU(), DOWN(), layers.Flatten(),
                layers.Dense(1)])
    assert net._gp_kinds() == ["conv", "resample", "resample", "conv", "resample", "dense"]


# ------------------------------------------------------------------ 3. models and demos
def _kinds(m):
    return [(type(l).__name__, s, tuple(l.out_shape(s))) for l, s in m.flat_layers()]


def _config(l):
    return {k: v for k, v in vars(l).items() if k not in ("vars", "name")}


def _swap(kinds, new, old):
    return [(old if n == new else n, s, o) for n, s, o in kinds]


@pytest.mark.parametrize("arch", ARCHS)
def test_default_and_existing_keywords_build_the_layer_lists_they_built(arch):
    for up in ("transpose", "resize"):
        a, b = models.DCGANGenerator(arch=arch, upsampling=up), models.DCGANGenerator(arch=arch, upsampling=up, resample_kernel=ASYM)
        assert _kinds(a) == _kinds(b) and [_config(l) for l in a.layers] == [_config(l) for l in b.layers]
        assert not any(l.kind in ("firup", "firdown") for l in a.layers)
        assert [l.kind for l in a.layers].count("upsample") == (0 if up == "transpose" else sum(1 for _, s, _ in models._G[arch][2] if s == 2))
    for down in ("stride", "pool"):
        a, b = models.DCGANDiscriminator(arch=arch, downsampling=down), models.DCGANDiscriminator(arch=arch, downsampling=down, resample_kernel=ASYM)
        assert _kinds(a) == _kinds(b) and [_config(l) for l in a.layers] == [_config(l) for l in b.layers]
        assert not any(l.kind in ("firup", "firdown") for l in a.layers)
        assert [l.kind for l in a.layers].count("avgpool") == (0 if down == "stride" else len(models._D[arch]))
    assert _kinds(models.DCGANGenerator(arch=arch)) == _kinds(models.DCGANGenerator(arch=arch, upsampling="transpose"))
    assert _kinds(models.DCGANDiscriminator(arch=arch)) == _kinds(models.DCGANDiscriminator(arch=arch, downsampling="stride"))
    with pytest.raises(ValueError, match="'filtered'"):
        models.DCGANGenerator(arch=arch, upsampling="bilinear")
    with pytest.raises(ValueError, match="'filtered'"):
        models.DCGANDiscriminator(arch=arch, downsampling="max")


@pytest.mark.parametrize("arch", ARCHS)
def test_filtered_stacks_equal_the_nearest_variants_in_everything_but_the_layer(arch):
    for make, new, old, twin_kw, kw in ((models.DCGANGenerator, "FilteredUpSampling2D", "UpSampling2D", dict(upsampling="resize"), dict(upsampling="filtered")),
                                        (models.DCGANDiscriminator, "FilteredDownSampling2D", "AveragePooling2D", dict(downsampling="pool"),
                                         dict(downsampling="filtered"))):
        twin, var = make(arch=arch, **twin_kw), make(arch=arch, resample_kernel=ASYM, **kw)
        assert _swap(_kinds(var), new, old) == _kinds(twin)                  # map sizes, layer order, the Dense input
        assert [n for n, _, _ in _kinds(var)].count(new) == [n for n, _, _ in _kinds(twin)].count(old) > 0
        assert all(l.taps == FR.normalized(ASYM) for l in var.layers if l.kind in ("firup", "firdown"))
        assert all(l.taps == FR.normalized((1, 3, 3, 1)) for l in make(arch=arch, **kw).layers if l.kind in ("firup", "firdown"))
        twin.build("cpu"), var.build("cpu")
        assert var.count_params() == twin.count_params() and len(var.variables) == len(twin.variables)
        assert [tuple(v.shape) for v in var.variables] == [tuple(v.shape) for v in twin.variables]
        swap = {"firup": "upsample", "firdown": "avgpool"}
        assert [swap.get(st.kind, st.kind) for st in var.net().stages] == [st.kind for st in twin.net().stages]
        assert var.output_shape == twin.output_shape
        for bad, err in (((1, 2, 1), NotImplementedError), ((1, -1), ValueError)):
            with pytest.raises(err):
                make(arch=arch, resample_kernel=bad, **kw)


def test_filtered_stacks_combine_with_the_other_keywords():
    d = models.DCGANDiscriminator(arch="tiny", downsampling="filtered", normalization="layer", minibatch_stddev=2, equalized_lr=True)
    d.build("cpu")
    assert [st.kind for st in d.net().stages] == ["conv", "firdown", "conv", "firdown", "mbstd", "dense"] and d.net().has_source
    g = models.DCGANGenerator(arch="tiny", upsampling="filtered", normalization="pixel", normalize_latents=True, spectral_norm=True)
    g.build("cpu")
    assert [st.kind for st in g.net().stages].count("firup") == 2 and g.net().has_pn


def test_models_docstring_names_the_keywords():
    assert 'upsampling="filtered"' in models.__doc__ and 'downsampling="filtered"' in models.__doc__ and "resample_kernel" in models.__doc__


def test_summary_and_the_averaged_twin_carry_the_kernel(capsys):
    g = models.DCGANGenerator(arch="tiny", upsampling="filtered", resample_kernel=ASYM)
    g.build("cpu")
    g.summary()
    out = capsys.readouterr().out
    assert "FilteredUpSampling2D" in out and f"Total params: {g.count_params():,}" in out
    twin = ema.clone_structure(g)
    assert _kinds(twin) == _kinds(g) and twin.count_params() == g.count_params()
    assert [st.kind for st in twin.net().stages] == [st.kind for st in g.net().stages]
    assert all(a is not b for a, b in zip(twin.layers, g.layers))
    fir = [(a, b) for a, b in zip(twin.layers, g.layers) if b.kind == "firup"]
    assert len(fir) == 2 and all(a.taps == b.taps == FR.normalized(ASYM) and a.resample_kernel == b.resample_kernel for a, b in fir)
    assert all(st.lin.taps == FR.normalized(ASYM) for st in twin.net().stages if st.kind == "firup")


def test_demos_take_the_switches():
    import demo_celeba
    import demo_mnist
    kinds = lambda m: [l.kind for l in m.layers]
    for demo in (demo_mnist, demo_celeba):
        args = demo.make_parser().parse_args([])
        assert (args.upsampling, args.downsampling, tuple(args.resample_kernel)) == ("transpose", "stride", (1, 3, 3, 1))
        args = demo.make_parser().parse_args(["--upsampling", "filtered", "--downsampling", "filtered", "--resample-kernel", "1,3,2,2"])
        assert (args.upsampling, args.downsampling, args.resample_kernel) == ("filtered", "filtered", (1.0, 3.0, 2.0, 2.0))
        for up in ("transpose", "resize"):
            assert kinds(demo.DCGANGenerator(upsampling=up, resample_kernel=ASYM)) == kinds(demo.DCGANGenerator(upsampling=up))
            assert "firup" not in kinds(demo.DCGANGenerator(upsampling=up))
        for down in ("stride", "pool"):
            assert kinds(demo.DCGANDiscriminator(downsampling=down, resample_kernel=ASYM)) == kinds(demo.DCGANDiscriminator(downsampling=down))
        g, gn = demo.DCGANGenerator(upsampling="filtered", resample_kernel=args.resample_kernel), demo.DCGANGenerator(upsampling="resize")
        d, dn = demo.DCGANDiscriminator(downsampling="filtered", resample_kernel=args.resample_kernel), demo.DCGANDiscriminator(downsampling="pool")
        assert [{"firup": "upsample"}.get(k, k) for k in kinds(g)] == kinds(gn) and kinds(g).count("firup") == kinds(gn).count("upsample") > 0
        assert [{"firdown": "avgpool"}.get(k, k) for k in kinds(d)] == kinds(dn) and kinds(d).count("firdown") == kinds(dn).count("avgpool") > 0
        assert all(l.taps == FR.normalized(ASYM) for l in g.layers + d.layers if l.kind in ("firup", "firdown"))
        assert g.output_shape == gn.output_shape and d.output_shape == dn.output_shape


# ------------------------------------------------------------------ 4. the reference operators
KERNELS = [(1, 1), (1, 3, 3, 1), (1, 3, 2, 2), (1, 2, 5, 3), (1, 5, 10, 10, 5, 1), (3, 1, 4, 1, 5, 9), (1, 2, 3, 4, 2, 2, 1, 1)]


@pytest.mark.parametrize("kernel", KERNELS)
def test_the_matrices_are_stylegan2s_upfirdn(kernel):
    """Zero-insert / pad / convolve / decimate with upsample_2d's and downsample_2d's padding rules, for sizes 1-8."""
    rng = np.random.default_rng(len(kernel))
    for n in range(1, 9):
        x, g = rng.normal(size=n), rng.normal(size=2 * n)
        np.testing.assert_allclose(FR.up_matrix(kernel, n) @ x, FR.stylegan2_up_1d(x, kernel), rtol=0, atol=1e-12)
        np.testing.assert_allclose(FR.down_matrix(kernel, n) @ g, FR.stylegan2_down_1d(g, kernel), rtol=0, atol=1e-12)


def test_the_box_kernel_is_nearest_upsampling_and_average_pooling():
    rng = np.random.default_rng(1)
    f = FR.normalized((1, 1))
    for shape in ((2, 3, 5, 4), (1, 1, 1, 3), (2, 4, 4, 1)):
        x = rng.integers(-64, 65, size=shape).astype(np.float64)
        hi = rng.integers(-64, 65, size=(shape[0], 2 * shape[1], 2 * shape[2], shape[3])).astype(np.float64)
        assert np.array_equal(FR.np_up(x, f, 4.0), x.repeat(2, 1).repeat(2, 2))
        assert np.array_equal(FR.np_down(hi, f), hi.reshape(shape[0], shape[1], 2, shape[2], 2, shape[3]).mean((2, 4)))
        assert np.array_equal(FR.np_up(x, f, 4.0, np.float32), x.repeat(2, 1).repeat(2, 2).astype(np.float32))


def test_the_default_kernel_is_half_pixel_bilinear_interpolation_in_the_interior():
    rng = np.random.default_rng(2)
    x = rng.normal(size=(2, 5, 7, 3))
    want = torch.nn.functional.interpolate(torch.as_tensor(x).permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=False)
    want = want.permute(0, 2, 3, 1).numpy()
    got = FR.np_up(x, FR.normalized((1, 3, 3, 1)), 4.0)
    np.testing.assert_allclose(got[:, 1:-1, 1:-1], want[:, 1:-1, 1:-1], rtol=0, atol=1e-14)
    assert np.abs(got[:, 0] - want[:, 0]).max() > 1e-3                      # the border is zero-padded, not edge-clamped
    np.testing.assert_allclose(FR.torch_firup(torch.as_tensor(x), FR.normalized((1, 3, 3, 1))).numpy(), got, rtol=0, atol=1e-14)


@pytest.mark.parametrize("kernel", KERNELS)
def test_the_adjoint_identity_holds_with_asymmetric_taps(kernel):
    rng = np.random.default_rng(3)
    t = FR.normalized(kernel)
    for shape in ((2, 1, 3, 2), (1, 3, 1, 1), (2, 4, 5, 3)):
        x = rng.integers(-8, 9, size=shape).astype(np.float64)
        g = rng.integers(-8, 9, size=(shape[0], 2 * shape[1], 2 * shape[2], shape[3])).astype(np.float64)
        lhs, rhs = (FR.np_up(x, t) * g).sum(), (x * FR.np_down(g, FR.flip(t))).sum()
        assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs))
        if t != FR.flip(t):
            assert abs(lhs - (x * FR.np_down(g, t)).sum()) > 1e-6          # the flip matters
        assert np.array_equal(FR.up_matrix(t, shape[1]).T, FR.down_matrix(FR.flip(t), shape[1]))


def test_the_torch_layers_differentiate_to_the_transposes():
    rng = np.random.default_rng(4)
    t = FR.normalized(ASYM)
    x = torch.as_tensor(rng.normal(size=(2, 3, 4, 2))).requires_grad_(True)
    g = rng.normal(size=(2, 6, 8, 2))
    dx, = torch.autograd.grad((FR.torch_firup(x, t) * torch.as_tensor(g)).sum(), x)
    np.testing.assert_allclose(dx.numpy(), FR.np_down(g, FR.flip(t), 4.0), rtol=0, atol=1e-13)
    h = torch.as_tensor(g).requires_grad_(True)
    dh, = torch.autograd.grad((FR.torch_firdown(h, t) * x.detach()).sum(), h)
    np.testing.assert_allclose(dh.numpy(), FR.np_up(x.detach().numpy(), FR.flip(t)), rtol=0, atol=1e-13)


# ------------------------------------------------------------------ 5. what the engine enqueues
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

    def named(self, name):
        return [a for n, a in self.events if n == name]


@contextlib.contextmanager
def recording(rec):
    saved = []

    def patch(obj, name, new):
        saved.append((obj, name, getattr(obj, name)))
        setattr(obj, name, new)

    for name, ret in dict(maker.RETURNS, fir_upsample2x="y", fir_downsample2x="y").items():
        patch(ops, name, rec.wrap(name, getattr(ops, name), ret))
    patch(bg.dist, "GradReducer", lambda *a, **k: rec)
    patch(layers, "default_device", lambda: torch.device("cpu"))
    try:
        yield rec
    finally:
        for obj, name, old in reversed(saved):
            setattr(obj, name, old)


def _same(a, b):
    return a.data_ptr() == b.data_ptr() and tuple(a.shape) == tuple(b.shape)


def test_launch_record_of_a_filtered_critic():
    """Forward: one bg_fir_downsample2x per stage with the layer's taps at scale 1.  Backward: one bg_fir_upsample2x per stage with the
    FLIPPED taps at scale 1 and the LeakyReLU' / Dropout' of the stage below in the same launch (ref = that stage's output, keep = its
    mask, its alpha and 1 / (1 - rate)); no mul_grad for those stages and none of the nearest pair's launches."""
    maker.ensure_library(ROOT)
    B = 2
    bg.layers.set_seed(3)
    disc = models.DCGANDiscriminator(arch="tiny", downsampling="filtered", resample_kernel=ASYM)
    disc.build("cpu")
    net = disc.net()
    fir = [i for i, st in enumerate(net.stages) if st.kind == "firdown"]
    assert fir == [1, 3]
    taps = FR.normalized(ASYM)
    rec = _Recorder()
    with recording(rec):
        ctx = net.context(B, "test")
        net.forward(ctx, torch.zeros(B, 8, 8, 3), training=True, seed=5)
        fwd = rec.named("fir_downsample2x")
        assert len(fwd) == len(fir) and not rec.named("fir_upsample2x") and not rec.named("pool2x_sum") and not rec.named("upsample2x")
        for i, a in zip(fir, fwd):
            assert a["taps"] == taps and a["scale"] == 1.0 and _same(a["x"], ctx.a[i - 1]) and a["y"] is ctx.a[i]
        del rec.events[:]
        net.backward(ctx, torch.zeros(B, 1), need_dx=True, need_dw=True)
        bwd = rec.named("fir_upsample2x")
        assert len(bwd) == len(fir) and not rec.named("fir_downsample2x") and not rec.named("mul_grad")
        for i, a in zip(reversed(fir), bwd):
            prev = net.stages[i - 1]
            assert a["taps"] == taps[::-1] != taps and a["scale"] == 1.0
            assert _same(a["x"], ctx.dz[i]) and _same(a["y"], ctx.dz[i - 1])
            assert _same(a["ref"], ctx.a[i - 1]) and _same(a["keep"], ctx.keep[i - 1])
            assert a["alpha"] == prev.alpha and a["grad_scale"] == prev.drop_scale == 1.0 / 0.7
        # inference (the G-step's critic pass): the same launch without a mask
        net.forward(ctx, torch.zeros(B, 8, 8, 3), training=False)
        del rec.events[:]
        net.backward(ctx, torch.zeros(B, 1), need_dx=True, need_dw=False)
        bwd = rec.named("fir_upsample2x")
        assert len(bwd) == len(fir) and not rec.named("mul_grad")
        assert all(a["keep"] is None and a["grad_scale"] == 1.0 and a["ref"] is not None and a["taps"] == taps[::-1] for a in bwd)
        # the merged pass: masks over the first 2B of 3B rows -> the masked rows, then the tail without a mask
        c3 = net.context(3 * B, "fr3", drop_rows=2 * B)
        net.forward(c3, torch.zeros(3 * B, 8, 8, 3), training=True, seed=5)
        del rec.events[:]
        net.backward(c3, torch.zeros(3 * B, 1), need_dx=True, need_dw=True, dw_rows=2 * B, dx_rows=(2 * B, 3 * B), defer_conv_dw=True)
        bwd = rec.named("fir_upsample2x")
        assert [a["x"].shape[0] for a in bwd] == [2 * B, B] * len(fir) and [a["keep"] is None for a in bwd] == [False, True] * len(fir)
        del rec.events[:]
        net.gp_second_order_merged(c3, 2 * B, 3 * B)
        tangent = rec.named("fir_downsample2x")                              # the penalty's linearised forward is the forward
        assert len(tangent) == len(fir) and all(a["taps"] == taps and a["scale"] == 1.0 and a["x"].shape[0] == B for a in tangent)
        assert not rec.named("fir_upsample2x")


def test_launch_record_of_a_filtered_generator():
    """Forward: one bg_fir_upsample2x per stage with the layer's taps at scale 4 and no ref; backward: one bg_fir_downsample2x per stage
    with the FLIPPED taps at scale 4."""
    maker.ensure_library(ROOT)
    B = 2
    bg.layers.set_seed(3)
    gen = models.DCGANGenerator(arch="tiny", upsampling="filtered", resample_kernel=ASYM)
    gen.build("cpu")
    net = gen.net()
    fir = [i for i, st in enumerate(net.stages) if st.kind == "firup"]
    assert len(fir) == 2
    taps = FR.normalized(ASYM)
    rec = _Recorder()
    with recording(rec):
        ctx = net.context(B, "test")
        net.forward(ctx, torch.zeros(B, 10), training=True)
        fwd = rec.named("fir_upsample2x")
        assert len(fwd) == len(fir) and not rec.named("fir_downsample2x") and not rec.named("upsample2x")
        for i, a in zip(fir, fwd):
            assert a["taps"] == taps and a["scale"] == 4.0 and a["ref"] is None and a["keep"] is None
            assert _same(a["x"], ctx.a[i - 1]) and a["y"] is ctx.a[i]
        del rec.events[:]
        net.backward(ctx, torch.zeros(B, 8, 8, 3), need_dx=False, need_dw=True)
        bwd = rec.named("fir_downsample2x")
        assert len(bwd) == len(fir) and not rec.named("fir_upsample2x") and not rec.named("pool2x_sum")
        for i, a in zip(reversed(fir), bwd):
            assert a["taps"] == taps[::-1] and a["scale"] == 4.0 and _same(a["x"], ctx.dz[i])


def test_launch_record_of_a_training_step():
    """A whole step of a filtered pair: per filtered stage and pass one launch each way (two where the merged pass splits masked rows
    and tail), and nothing of the nearest pair."""
    maker.ensure_library(ROOT)
    rec = _Recorder()
    with recording(rec):
        bg.layers.set_seed(3)
        gen = models.DCGANGenerator(arch="tiny", upsampling="filtered")
        disc = models.DCGANDiscriminator(arch="tiny", downsampling="filtered")
        gen.build("cpu"), disc.build("cpu")
        gan = bg.WGANGP(gen, disc, bg.WGANGP.HyperParameters(batch_size=2, global_batch_size=2), bg.TrainingConfig(log_dir=os.devnull),
                        step_replay=False)
        gan.train_on_batch(np.zeros((2, 8, 8, 3), np.float32))
    names = [n for n, _ in rec.events]
    # up: G inference 2 + merged critic backward 2 x (masked, tail) + G-step generator forward 2 + G-step critic backward 2
    # down: merged critic forward 2 + penalty tangent 2 + G-step critic forward 2 + generator backward 2
    assert names.count("fir_upsample2x") == 10 and names.count("fir_downsample2x") == 8
    assert "upsample2x" not in names and "pool2x_sum" not in names


def test_nearest_stacks_enqueue_none_of_it():
    maker.ensure_library(ROOT)
    rec = _Recorder()
    with recording(rec):
        bg.layers.set_seed(3)
        gen, disc = models.DCGANGenerator(arch="tiny", upsampling="resize"), models.DCGANDiscriminator(arch="tiny", downsampling="pool")
        gen.build("cpu"), disc.build("cpu")
        gan = bg.WGANGP(gen, disc, bg.WGANGP.HyperParameters(batch_size=2, global_batch_size=2), bg.TrainingConfig(log_dir=os.devnull),
                        step_replay=False)
        gan.train_on_batch(np.zeros((2, 8, 8, 3), np.float32))
    names = [n for n, _ in rec.events]
    assert not [n for n in names if n.startswith("fir_")] and names.count("upsample2x") == 10 and names.count("pool2x_sum") == 8


# ------------------------------------------------------------------ 6. ABI
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge._load_build_module().build_lib(verbose=False)
    from blurred_gan_amd import _lib
    return _lib.load()


def test_argument_errors_are_statuses_and_launch_nothing(lib):
    from blurred_gan_amd import _lib
    assert "bg_fir_upsample2x_nhwc_f32" in _lib.SIGNATURES and "bg_fir_downsample2x_nhwc_f32" in _lib.SIGNATURES
    buf = np.zeros(320, np.float32)
    base = buf.ctypes.data
    base += (-base) % 16                               # 16-byte aligned host addresses: never dereferenced by the checks
    x, y, r, k, t = base, base + 64, base + 512, base + 768, base + 1024
    up, down = lib.bg_fir_upsample2x_nhwc_f32, lib.bg_fir_downsample2x_nhwc_f32
    NULL, SHAPE, ALIGN = -6, -1, -2
    assert up(None, y, 1, 1, 1, 4, t, 4, 1.0, None, None, 0.3, 1.0, None) == NULL
    assert up(x, None, 1, 1, 1, 4, t, 4, 1.0, None, None, 0.3, 1.0, None) == NULL
    assert up(x, y, 1, 1, 1, 4, None, 4, 1.0, None, None, 0.3, 1.0, None) == NULL
    assert up(x, y, 1, 1, 1, 4, t, 4, 1.0, None, k, 0.3, 1.0, None) == NULL          # a keep mask without ref
    assert b"bg_fir_upsample2x_nhwc_f32" in lib.bg_last_error()
    assert down(None, y, 1, 1, 1, 4, t, 4, 1.0, None) == NULL
    assert down(x, None, 1, 1, 1, 4, t, 4, 1.0, None) == NULL
    assert down(x, y, 1, 1, 1, 4, None, 4, 1.0, None) == NULL
    assert b"bg_fir_downsample2x_nhwc_f32" in lib.bg_last_error()
    for dims in ((0, 1, 1, 4), (1, 0, 1, 4), (1, 1, 0, 4), (1, 1, 1, 0), (-1, 1, 1, 4), (1, 1, -2, 4), (1, 1, 1, -4)):
        assert up(x, y, *dims, t, 4, 1.0, None, None, 0.3, 1.0, None) == SHAPE
        assert up(x, y, *dims, t, 4, 1.0, r, k, 0.3, 1.0, None) == SHAPE
        assert down(x, y, *dims, t, 4, 1.0, None) == SHAPE
    for n_taps in (0, 1, 3, 5, 7, 9, 10, 16, -2, -4):
        assert up(x, y, 1, 1, 1, 4, t, n_taps, 1.0, None, None, 0.3, 1.0, None) == SHAPE
        assert down(x, y, 1, 1, 1, 3, t, n_taps, 1.0, None) == SHAPE
        assert b"n_taps" in lib.bg_last_error()
    for C in (4, 20):
        assert up(x + 4, y, 1, 1, 1, C, t, 4, 1.0, None, None, 0.3, 1.0, None) == ALIGN
        assert up(x, y + 8, 1, 1, 1, C, t, 4, 1.0, None, None, 0.3, 1.0, None) == ALIGN
        assert up(x, y, 1, 1, 1, C, t, 4, 1.0, r + 12, None, 0.3, 1.0, None) == ALIGN
        assert up(x, y, 1, 1, 1, C, t, 4, 1.0, r, k + 4, 0.3, 1.0, None) == ALIGN
        assert up(x, y, 1, 1, 1, C, t, 4, 1.0, r, k + 1, 0.3, 1.0, None) == ALIGN
        assert b"aligned" in lib.bg_last_error()
        assert down(x + 4, y, 1, 1, 1, C, t, 4, 1.0, None) == ALIGN
        assert down(x, y + 12, 1, 1, 1, C, t, 4, 1.0, None) == ALIGN
        assert b"aligned" in lib.bg_last_error()
    assert lib.bg_version() == 5                       # an addition: the ABI version stays
    assert not buf.any()
    with pytest.raises(ops.BgDeviceError):             # the wrappers refuse host tensors before anything is launched
        ops.fir_upsample2x(torch.zeros(1, 1, 1, 4), torch.zeros(1, 2, 2, 4), (0.5, 0.5))
    with pytest.raises(ops.BgDeviceError):
        ops.fir_downsample2x(torch.zeros(1, 2, 2, 4), torch.zeros(1, 1, 1, 4), (0.5, 0.5))
    with pytest.raises(AssertionError):                # the shape assertions of ops.upsample2x / ops.pool2x_sum
        ops.fir_upsample2x(torch.zeros(1, 1, 1, 4), torch.zeros(1, 2, 3, 4), (0.5, 0.5))
    with pytest.raises(AssertionError):
        ops.fir_downsample2x(torch.zeros(1, 2, 2, 4), torch.zeros(1, 1, 2, 4), (0.5, 0.5))
