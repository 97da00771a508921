"""CPU tests of the resampling layers (layers.UpSampling2D / AveragePooling2D, engine placement rules, the "resize" / "pool"
variants of the DCGAN stacks) and of the argument checks of bg_upsample2x_nhwc_f32 / bg_pool2x_sum_nhwc_f32 (no device work
is launched)."""
import numpy as np
import pytest

import blurred_gan_amd as bg
from blurred_gan_amd import layers, models
from blurred_gan_amd.engine import Net

ARCHS = sorted(models.IMAGE_SHAPE)


# ------------------------------------------------------------------ layers
def test_shape_arithmetic():
    up, pool = layers.UpSampling2D(), layers.AveragePooling2D()
    assert (up.kind, pool.kind) == ("upsample", "avgpool")
    assert up.out_shape((3, 5, 7)) == (6, 10, 7) and up.out_shape((1, 1, 1)) == (2, 2, 1)
    assert pool.out_shape((6, 10, 7)) == (3, 5, 7) and pool.out_shape((2, 2, 1)) == (1, 1, 1)
    assert pool.out_shape(up.out_shape((4, 9, 2))) == (4, 9, 2)
    for l in (up, pool):
        assert l.var_specs((4, 4, 8)) == [] and l.vars == {} and l.count_params() == 0


def test_accepted_arguments():
    layers.UpSampling2D(2)
    layers.UpSampling2D(size=(2, 2), data_format="channels_last", interpolation="nearest")
    layers.AveragePooling2D(2)
    layers.AveragePooling2D(pool_size=(2, 2), strides=2, padding="valid", data_format="channels_last")
    layers.AveragePooling2D(strides=(2, 2))
    layers.AveragePooling2D(strides=None)


@pytest.mark.parametrize("make", [lambda: layers.UpSampling2D(3), lambda: layers.UpSampling2D((2, 1)), lambda: layers.UpSampling2D((4, 4)),
                                  lambda: layers.UpSampling2D(interpolation="bilinear"),
                                  lambda: layers.UpSampling2D(data_format="channels_first"),
                                  lambda: layers.AveragePooling2D(3), lambda: layers.AveragePooling2D((2, 4)),
                                  lambda: layers.AveragePooling2D(strides=1), lambda: layers.AveragePooling2D(strides=(2, 1)),
                                  lambda: layers.AveragePooling2D(data_format="channels_first")])
def test_argument_refusals(make):
    with pytest.raises(NotImplementedError):
        make()


@pytest.mark.parametrize("shape", [(5, 4, 2), (4, 7, 2), (3, 3, 1)])
def test_pooling_an_odd_map_is_refused_when_shapes_are_inferred(shape):
    with pytest.raises(NotImplementedError, match="odd"):
        layers.AveragePooling2D().out_shape(shape)
    with pytest.raises(NotImplementedError, match="odd"):
        layers.Sequential([layers.Conv2D(4, 3, padding="same", input_shape=list(shape)), layers.AveragePooling2D()])


# ------------------------------------------------------------------ placement (engine.Net.__init__)
def _net(ls):
    m = layers.Sequential(ls)
    m.build("cpu")
    return Net(m.flat_layers(), m.store)


def _conv(**kw):
    return layers.Conv2D(4, 3, padding="same", **kw)


@pytest.mark.parametrize("resample", [layers.UpSampling2D, layers.AveragePooling2D])
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


def test_allowed_placements_compile_into_stages_of_their_own():
    net = _net([_conv(input_shape=(4, 4, 2)), layers.LeakyReLU(), layers.Dropout(0.3), layers.AveragePooling2D(),
                layers.UpSampling2D(), _conv(), layers.BatchNormalization(), layers.LeakyReLU(), layers.UpSampling2D(),
                layers.AveragePooling2D(), layers.Flatten(), layers.Dense(1)])
    assert [st.kind for st in net.stages] == ["conv", "avgpool", "upsample", "conv", "upsample", "avgpool", "dense"]
    assert [st.out_shape for st in net.stages] == [(4, 4, 4), (2, 2, 4), (4, 4, 4), (4, 4, 4), (8, 8, 4), (4, 4, 4), (1,)]
    assert len(net.conv_layers) == 2
    for st in net.stages:
        if st.kind in ("avgpool", "upsample"):
            assert st.bn is None and st.act is None and not st.drop and not st.fusable_grad
            assert net.store.train_range(st.lin, st.bn) == (0, 0)
    assert net.stages[0].fusable_grad            # the pooling stage's backward lands as this stage's dz
    ctx = net.context(3)
    assert ctx.keep[1] is None and ctx.z[1] is None and tuple(ctx.a[1].shape) == (3, 2, 2, 4)


# ------------------------------------------------------------------ models
def _kinds(m):
    return [(type(l).__name__, s, tuple(l.out_shape(s))) for l, s in m.flat_layers()]


def _config(l):
    return {k: v for k, v in vars(l).items() if k not in ("vars", "name")}


@pytest.mark.parametrize("arch", ARCHS)
def test_default_keywords_build_the_default_layer_lists(arch):
    for a, b in ((models.DCGANGenerator(arch=arch), models.DCGANGenerator(arch=arch, upsampling="transpose")),
                 (models.DCGANDiscriminator(arch=arch), models.DCGANDiscriminator(arch=arch, downsampling="stride"))):
        assert _kinds(a) == _kinds(b)
        assert [_config(l) for l in a.layers] == [_config(l) for l in b.layers]
        assert not any(l.kind in ("upsample", "avgpool") for l in a.layers)
    with pytest.raises(ValueError):
        models.DCGANGenerator(arch=arch, upsampling="bilinear")
    with pytest.raises(ValueError):
        models.DCGANDiscriminator(arch=arch, downsampling="max")


@pytest.mark.parametrize("arch", ARCHS)
def test_resize_generator_keeps_map_sizes_and_parameter_count(arch):
    base, var = models.DCGANGenerator(arch=arch), models.DCGANGenerator(arch=arch, upsampling="resize")
    assert var.output_shape == base.output_shape == (None,) + models.IMAGE_SHAPE[arch]
    n_up = 0
    it = iter(var.layers)
    for l in base.layers:
        v = next(it)
        if l.kind == "convT" and l.stride == 2:
            assert v.kind == "upsample"
            n_up += 1
            v = next(it)
            assert v.kind == "conv" and (v.filters, v.k, v.stride, v.use_bias, v.activation) == (l.filters, l.k, 1, l.use_bias, l.activation)
        else:
            assert type(v) is type(l) and _config(v) == _config(l)
    assert next(it, None) is None and n_up == sum(1 for _, s, _ in models._G[arch][2] if s == 2) > 0
    # the maps behind every learned layer are the default variant's
    maps = lambda m: [o for n, _, o in _kinds(m) if n not in ("UpSampling2D",)]
    assert maps(var) == maps(base)
    base.build("cpu"), var.build("cpu")
    assert var.count_params() == base.count_params() and len(var.variables) == len(base.variables)
    assert [st.kind for st in var.net().stages].count("upsample") == n_up


@pytest.mark.parametrize("arch", ARCHS)
def test_pooled_critic_keeps_map_sizes_parameter_count_and_dense_input(arch):
    base, var = models.DCGANDiscriminator(arch=arch), models.DCGANDiscriminator(arch=arch, downsampling="pool")
    kb, kv = _kinds(base), _kinds(var)
    assert [n for n, _, _ in kv] == ["Conv2D", "LeakyReLU", "Dropout", "AveragePooling2D"] * len(models._D[arch]) + ["Flatten", "Dense"]
    pooled = [o for n, _, o in kv if n == "AveragePooling2D"]
    assert pooled == [o for n, _, o in kb if n == "Dropout"]                  # same map behind every block
    assert all(s[0] % 2 == 0 and s[1] % 2 == 0 for n, s, _ in kv if n == "AveragePooling2D")
    assert [s for n, s, _ in kv if n == "Dense"] == [s for n, s, _ in kb if n == "Dense"]
    assert all(l.stride == 1 for l in var.layers if l.kind == "conv")
    base.build("cpu"), var.build("cpu")
    assert var.count_params() == base.count_params()
    assert [tuple(v.shape) for v in var.variables] == [tuple(v.shape) for v in base.variables]
    assert [st.kind for st in var.net().stages] == ["conv", "avgpool"] * len(models._D[arch]) + ["dense"]


def test_summary_checkpoint_keys_and_the_averaged_twin_need_no_special_case(capsys):
    from blurred_gan_amd import ema
    g = models.DCGANGenerator(arch="tiny", upsampling="resize")
    g.build("cpu")
    g.summary()
    out = capsys.readouterr().out
    assert "UpSampling2D" in out and f"Total params: {g.count_params():,}" in out
    twin = ema.clone_structure(g)
    assert _kinds(twin) == _kinds(g) and twin.count_params() == g.count_params()
    assert [st.kind for st in twin.net().stages] == [st.kind for st in g.net().stages]
    assert all(a is not b for a, b in zip(twin.layers, g.layers))
    w = g.get_weights()
    twin.set_weights(w)
    assert all(np.array_equal(a, b) for a, b in zip(twin.get_weights(), w))


# ------------------------------------------------------------------ ABI
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge._load_build_module().build_lib(verbose=False)
    from blurred_gan_amd import _lib
    return _lib.load()


def test_argument_errors_are_statuses_and_launch_nothing(lib):
    from blurred_gan_amd import _lib
    assert "bg_upsample2x_nhwc_f32" in _lib.SIGNATURES and "bg_pool2x_sum_nhwc_f32" in _lib.SIGNATURES
    buf = np.zeros(256, np.float32)
    base = buf.ctypes.data
    base += (-base) % 16                               # 16-byte aligned host addresses: never dereferenced by the checks
    x, y, r, k = base, base + 64, base + 512, base + 768
    up, pool = lib.bg_upsample2x_nhwc_f32, lib.bg_pool2x_sum_nhwc_f32
    NULL, SHAPE, ALIGN = -6, -1, -2
    assert up(None, y, 1, 1, 1, 4, 1.0, None, None, 0.3, 1.0, None) == NULL
    assert up(x, None, 1, 1, 1, 4, 1.0, None, None, 0.3, 1.0, None) == NULL
    assert up(x, y, 1, 1, 1, 4, 1.0, None, k, 0.3, 1.0, None) == NULL          # a keep mask without ref
    assert b"bg_upsample2x_nhwc_f32" in lib.bg_last_error()
    assert pool(None, y, 1, 1, 1, 4, 1.0, None) == NULL
    assert pool(x, None, 1, 1, 1, 4, 1.0, None) == NULL
    assert b"bg_pool2x_sum_nhwc_f32" in lib.bg_last_error()
    for dims in ((0, 1, 1, 4), (1, 0, 1, 4), (1, 1, 0, 4), (1, 1, 1, 0), (-1, 1, 1, 4), (1, 1, -2, 4), (1, 1, 1, -4)):
        assert up(x, y, *dims, 1.0, None, None, 0.3, 1.0, None) == SHAPE
        assert up(x, y, *dims, 1.0, r, k, 0.3, 1.0, None) == SHAPE
        assert pool(x, y, *dims, 1.0, None) == SHAPE
    for C in (4, 20):
        assert up(x + 4, y, 1, 1, 1, C, 1.0, None, None, 0.3, 1.0, None) == ALIGN
        assert up(x, y + 8, 1, 1, 1, C, 1.0, None, None, 0.3, 1.0, None) == ALIGN
        assert up(x, y, 1, 1, 1, C, 1.0, r + 12, None, 0.3, 1.0, None) == ALIGN
        assert up(x, y, 1, 1, 1, C, 1.0, r, k + 4, 0.3, 1.0, None) == ALIGN
        assert up(x, y, 1, 1, 1, C, 1.0, r, k + 1, 0.3, 1.0, None) == ALIGN
        assert b"aligned" in lib.bg_last_error()
        assert pool(x + 4, y, 1, 1, 1, C, 1.0, None) == ALIGN
        assert pool(x, y + 12, 1, 1, 1, C, 1.0, None) == ALIGN
        assert b"aligned" in lib.bg_last_error()
    assert lib.bg_version() == 5                       # an addition: the ABI version stays
    assert not buf.any()
