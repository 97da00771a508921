"""CPU tests of layers.EqualizedLearningRate: the layer surface, its coefficient and initialiser, the refusals, the DCGAN stacks'
``equalized_lr=`` argument, the host side of the bg_eqlr_* entry points, the averaged model's clone, the checkpoint signature and
what a step of wrapped models enqueues."""
import contextlib
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import blurred_gan_amd as bg
from blurred_gan_amd import _lib, ema, layers, models, ops
from blurred_gan_amd.checkpoint import CheckpointManager
from test_spectral_cpu import ROOT, _Recorder, maker, recording

EQ = layers.EqualizedLearningRate
SQRT2 = math.sqrt(2)


def _coefficient(gain, fan_in):
    """The formula in double, rounded to fp32 once."""
    return float(np.float32(np.float64(gain) / np.sqrt(np.float64(fan_in))))


# ------------------------------------------------------------------ 1. the layer surface
def _wrapped_stack():
    return layers.Sequential([
        EQ(layers.Conv2D(8, 3, strides=2, padding="same", input_shape=[8, 8, 3])),
        layers.LeakyReLU(),
        EQ(layers.Conv2DTranspose(4, 5, strides=2, padding="same", use_bias=False), gain=1.0),
        layers.LeakyReLU(),
        layers.Flatten(),
        EQ(layers.Dense(2), gain=2),
    ])


def test_wrapper_stands_for_the_layer_it_wraps():
    m = _wrapped_stack().build("cpu")
    names = [(n, tuple(sh), tr) for (_, n, _, sh, tr) in m.store.entries]
    assert names == [("kernel", (3, 3, 3, 8), True), ("bias", (8,), True), ("kernel", (5, 5, 4, 8), True), ("kernel", (256, 2), True), ("bias", (2,), True)]
    assert m.store.n_state == 0 and m.count_params() == 216 + 8 + 800 + 512 + 2 and m.output_shape == (None, 2)
    w = m.layers[0]
    assert w.kind == "conv" and w.filters == 8 and w.k == 3 and w.stride == 2 and w.layer.vars is w.vars and w.name.startswith("equalized_learning_rate_")
    assert [l.kind for l in m.layers if isinstance(l, EQ)] == ["conv", "convT", "dense"]
    assert [l.gain for l in m.layers if isinstance(l, EQ)] == [SQRT2, 1.0, 2.0]
    assert [l.fan_in for l in m.layers if isinstance(l, EQ)] == [27, 25 * 8, 256]
    net = m.net()
    assert net.eqlr_layers == [m.layers[0], m.layers[2], m.layers[5]] and net.plain_conv_layers == [] and net.spectral_layers == []
    assert [st.kind for st in net.stages] == ["conv", "convT", "dense"] and [st.act for st in net.stages] == ["lrelu", "lrelu", None]


@pytest.mark.parametrize("make,shape,fan_in", [
    (lambda: layers.Dense(68, input_shape=(12,)), (12, 68), 12),
    (lambda: layers.Conv2D(16, 5, padding="same", input_shape=[8, 8, 3]), (5, 5, 3, 16), 75),
    (lambda: layers.Conv2DTranspose(16, 5, strides=2, padding="same", input_shape=[4, 4, 32]), (5, 5, 16, 32), 800),
])
@pytest.mark.parametrize("gain", [SQRT2, 1.0, 0.37])
def test_coefficient_is_the_double_formula_rounded_once(make, shape, fan_in, gain):
    w = EQ(make(), gain=gain)
    m = layers.Sequential([w])
    assert w.coefficient == _coefficient(gain, fan_in) and w.fan_in == fan_in       # known once the input shape is
    m.build("cpu")
    assert tuple(w.vars["kernel"].shape) == shape and EQ.fan_in_of(w.kind, shape) == fan_in
    assert isinstance(w.coefficient, float) and w.coefficient == _coefficient(gain, fan_in) == float(np.float32(w.coefficient))


def test_initial_kernel_is_standard_normal_from_the_seed_stream_and_the_bias_zero():
    bg.set_seed(17)
    m = layers.Sequential([EQ(layers.Dense(512, input_shape=(256,))), layers.Reshape((8, 8, 8)), EQ(layers.Conv2D(64, 5, padding="same"))]).build("cpu")
    for l in m.layers:
        if not isinstance(l, EQ):
            continue
        k = l.vars["kernel"].numpy().astype(np.float64)
        n = k.size
        assert n >= 12800
        assert abs(k.mean()) <= 5 / math.sqrt(n), k.mean()                       # standard error of the mean: 1 / sqrt(n)
        assert abs(k.std() - 1) <= 5 / math.sqrt(2 * n), k.std()                # of the standard deviation: 1 / sqrt(2 n)
        assert not l.vars["bias"].numpy().any()
    bg.set_seed(17)
    again = layers.Sequential([EQ(layers.Dense(512, input_shape=(256,)))]).build("cpu")
    assert torch.equal(again.layers[0].vars["kernel"], m.layers[0].vars["kernel"])
    bg.set_seed(17)
    assert np.array_equal(m.layers[0].vars["kernel"].numpy(), layers._seed_state["rng"].standard_normal((256, 512)).astype(np.float32))


# ------------------------------------------------------------------ 2. refusals
def test_refusals():
    for bad in (layers.LeakyReLU(), layers.BatchNormalization(), layers.LayerNormalization(), layers.Flatten(), layers.UpSampling2D(),
                layers.PixelNormalization(), layers.Sequential()):
        with pytest.raises(NotImplementedError, match="wraps a Conv2D"):
            EQ(bad)
    with pytest.raises(NotImplementedError, match="cancels"):
        EQ(layers.SpectralNormalization(layers.Dense(3)))
    with pytest.raises(NotImplementedError, match="cancels"):
        layers.SpectralNormalization(EQ(layers.Dense(3)))
    with pytest.raises(NotImplementedError, match="wraps a Conv2D"):
        EQ(EQ(layers.Dense(3)))
    for gain in (0, 0.0, -1.0, float("inf"), float("nan"), None, "2", True):
        with pytest.raises(ValueError, match="gain"):
            EQ(layers.Dense(3), gain=gain)
    both = layers.Sequential([EQ(layers.Conv2D(8, 3, padding="same", input_shape=[4, 4, 3])), layers.LeakyReLU(), layers.Flatten(),
                              layers.SpectralNormalization(layers.Dense(1))]).build("cpu")
    with pytest.raises(NotImplementedError, match="effective-weight buffer"):
        both.net()


def test_the_stacks_refuse_both_wrappers_together():
    import demo_celeba
    import demo_mnist
    for cls in (models.DCGANGenerator, models.DCGANDiscriminator, demo_mnist.DCGANGenerator, demo_mnist.DCGANDiscriminator,
                demo_celeba.DCGANGenerator, demo_celeba.DCGANDiscriminator):
        with pytest.raises(ValueError, match="equalized_lr"):
            cls(equalized_lr=True, spectral_norm=True)


# ------------------------------------------------------------------ 3. models and demos
def _expected_gain(flat, i):
    """sqrt(2) in front of a LeakyReLU, 1 for a fused tanh or a linear head; reads the layer list alone."""
    l = flat[i]
    if getattr(l, "activation", None) == "tanh":
        return 1.0
    for nxt in flat[i + 1:]:
        if nxt.kind == "lrelu":
            return SQRT2
        if nxt.kind in ("dense", "conv", "convT"):
            break
    return 1.0


GEN_KW = [{}, dict(upsampling="resize"), dict(normalization="pixel"), dict(normalization="pixel", normalize_latents=True, upsampling="resize")]
DISC_KW = [{}, dict(downsampling="pool"), dict(normalization="layer"), dict(minibatch_stddev=2), dict(downsampling="pool", normalization="layer", minibatch_stddev=4)]


@pytest.mark.parametrize("arch", ["tiny", "tiny_mnist", "celeba64"])
def test_model_layer_lists_and_gains(arch):
    for cls, kws in ((models.DCGANGenerator, GEN_KW), (models.DCGANDiscriminator, DISC_KW)):
        for kw in kws:
            plain, eq = cls(arch=arch, **kw), cls(arch=arch, equalized_lr=True, **kw)
            fp, fe = [l for l, _ in plain.flat_layers()], [l for l, _ in eq.flat_layers()]
            assert [l.kind for l in fp] == [l.kind for l in fe]
            lin = [i for i, l in enumerate(fe) if l.kind in ("dense", "conv", "convT")]
            assert lin and all(isinstance(fe[i], EQ) and type(fe[i].layer) is type(fp[i]) for i in lin)
            assert not any(isinstance(l, EQ) for l in fp)
            assert [fe[i].gain for i in lin] == [_expected_gain(fe, i) for i in lin], (cls.__name__, kw)
            gains = [fe[i].gain for i in lin]
            assert gains[-1] == 1.0 and all(g == SQRT2 for g in gains[:-1])          # only the tanh layer / the Dense(1) head has gain 1
            for i in lin:
                l, shape = fe[i], [sh for n, sh, _, _ in fe[i].var_specs(eq.flat_layers()[i][1]) if n == "kernel"][0]
                assert l.coefficient == _coefficient(l.gain, EQ.fan_in_of(l.kind, shape))
            assert [[(n, sh, tr) for n, sh, tr, _ in l.var_specs(s)] for l, s in plain.flat_layers()] == \
                   [[(n, sh, tr) for n, sh, tr, _ in l.var_specs(s)] for l, s in eq.flat_layers()]


TINY_G = (['Dense', 'BatchNormalization', 'LeakyReLU', 'Reshape', 'Conv2DTranspose', 'BatchNormalization', 'LeakyReLU', 'Conv2DTranspose',
           'BatchNormalization', 'LeakyReLU', 'Conv2DTranspose', 'BatchNormalization', 'LeakyReLU', 'Conv2D'],
          [(10, 128), (128,), (128,), (128,), (128,), (5, 5, 32, 32), (32,), (32,), (32,), (32,), (5, 5, 16, 32), (16,), (16,), (16,), (16,),
           (5, 5, 16, 16), (16,), (16,), (16,), (16,), (5, 5, 16, 3)])
TINY_D = (['Conv2D', 'LeakyReLU', 'Dropout', 'Conv2D', 'LeakyReLU', 'Dropout', 'Flatten', 'Dense'], [(5, 5, 3, 16), (16,), (5, 5, 16, 32), (32,), (128, 1), (1,)])


def test_default_stacks_are_built_variable_for_variable_as_before():
    for cls, (names, shapes) in ((models.DCGANGenerator, TINY_G), (models.DCGANDiscriminator, TINY_D)):
        built = []
        for kw in ({}, dict(equalized_lr=False)):
            bg.set_seed(9)
            m = cls(arch="tiny", **kw).build("cpu")
            assert [type(l).__name__ for l in m._own_layers()] == names and [tuple(sh) for (_, _, _, sh, _) in m.store.entries] == shapes
            assert m.store.eff is None and m.store._eq_table is None and m.net().eqlr_layers == [] and m.net().plain_conv_layers == m.net().conv_layers
            built.append(m.get_weights())
        assert all(np.array_equal(a, b) for a, b in zip(*built))
        for l in m._own_layers():               # Glorot uniform as before, not the normal draw
            if l.kind in ("dense", "conv", "convT"):
                k = l.vars["kernel"].numpy()
                sh = k.shape
                rf = int(np.prod(sh[:-2])) if len(sh) == 4 else 1
                assert np.abs(k).max() <= math.sqrt(6.0 / (rf * sh[-2] + rf * sh[-1]))


def test_demos_take_the_flags():
    import demo_celeba
    import demo_mnist
    for demo in (demo_mnist, demo_celeba):
        off = demo.make_parser().parse_args([])
        assert off.critic_equalized_lr is False and off.generator_equalized_lr is False
        on = demo.make_parser().parse_args(["--critic-equalized-lr", "--generator-equalized-lr"])
        assert on.critic_equalized_lr is True and on.generator_equalized_lr is True
        for cls in (demo.DCGANDiscriminator, demo.DCGANGenerator):
            wrapped = lambda m: [isinstance(l, EQ) for l in m.layers if l.kind in ("dense", "conv", "convT")]
            assert not any(wrapped(cls())) and all(wrapped(cls(equalized_lr=True))) and wrapped(cls(equalized_lr=True))
            gains = [l.gain for l in cls(equalized_lr=True).layers if isinstance(l, EQ)]
            assert gains[-1] == 1.0 and all(g == SQRT2 for g in gains[:-1])


# ------------------------------------------------------------------ 4. the host side of the entry points
SHAPES = [(130, 1, 1), (12, 68, 1), (9 * 68, 132, 9), (64, 64, 1), (16, 8, 4), (75, 5, 25), (25, 4, 25), (12800, 512, 25), (16384, 1, 1), (16385, 1, 1)]


def test_plan_against_a_restatement():
    maker.ensure_library(ROOT)
    unit = ops.eqlr.plan(1, 1)["unit_elems"]
    assert unit > 0 and unit % 1024 == 0               # 256 threads x whole float4 trips
    for K, N, taps in SHAPES:
        R = K // taps
        want = dict(tiles=taps * -(-R // 64) * -(-N // 64), vec=4 if R % 4 == 0 and N % 4 == 0 else 1, grad_units=-(-K * N // unit), unit_elems=unit)
        assert ops.eqlr.plan(K, N, taps) == want, (K, N, taps)
    for bad in ((0, 4, 1), (4, 0, 1), (4, 4, 0), (10, 4, 3), (1 << 15, 1 << 15, 1)):
        with pytest.raises(ValueError, match="BAD_SHAPE|shape"):
            ops.eqlr.plan(*bad)


def _table(shapes=((75, 16, 25), (128, 1, 1), (100, 8, 25)), c=0.125):
    rows, off_t, off_e = [], 0, 0
    pad = lambda n: -(-n // 4) * 4
    for K, N, taps in shapes:
        rows.append(dict(w_off=off_t, eff_off=off_e, tr_off=off_e + pad(K * N) if taps > 1 else -1, K=K, N=N, taps=taps, c=c))
        off_t, off_e = off_t + pad(K * N), off_e + (2 if taps > 1 else 1) * pad(K * N)
    return np.ascontiguousarray(ops.eqlr.rows(rows), dtype=np.int32), off_t, off_e


def test_table_checker_refuses_bad_tables_before_anything_is_launched():
    maker.ensure_library(ROOT)
    lib = _lib.load()
    good, nt, ne = _table()
    assert good.shape == (3, _lib.EQLR_DESC_INTS) and good[:, 8].view(np.float32).tolist() == [0.125] * 3
    ops.eqlr.check_table(good, nt, ne)
    NULL, SHAPE, ALIGN = -6, -1, -2
    buf = np.full(64 + 4, 7.0, np.float32)          # host memory standing in for the bases: a refused call never dereferences them
    base = buf.ctypes.data
    base += (-base) % 16

    def statuses(t, n=None, theta_floats=nt, eff_floats=ne):
        p, n = (None if t is None else t.ctypes.data), (len(good) if n is None else n)
        return {lib.bg_eqlr_check_table(p, n, theta_floats, eff_floats), lib.bg_eqlr_scale_f32(base, theta_floats, base, eff_floats, base, p, n, None),
                lib.bg_eqlr_grad_f32(base, theta_floats, base, p, n, None)}

    def edited(row, col, val, add=False):
        t = good.copy()
        t[row, col] = t[row, col] + val if add else val
        return t

    assert statuses(None) == {NULL} and statuses(good, n=0) == {SHAPE} and statuses(good, n=-1) == {SHAPE}
    for col in (0, 1, 2):                                   # a misaligned offset: w_off, eff_off, tr_off
        assert statuses(edited(0, col, 2, add=True)) == {ALIGN}, col
        with pytest.raises(ValueError, match="multiples of 4"):
            ops.eqlr.check_table(edited(0, col, 2, add=True), nt, ne)
    for row, col, val in ((1, 0, 0),                        # layer 1's kernel on layer 0's
                          (1, 1, 0),                        # layer 1's effective kernel on layer 0's
                          (2, 2, int(good[0, 2])),          # layer 2's transposed copy on layer 0's
                          (2, 1, int(good[0, 2]) + 4),      # layer 2's effective kernel inside layer 0's transposed copy
                          (0, 2, int(good[0, 1]) + 8)):     # a layer's transposed copy inside its own effective kernel
        assert statuses(edited(row, col, val)) == {SHAPE}, (row, col)
        with pytest.raises(ValueError, match="overlap"):
            ops.eqlr.check_table(edited(row, col, val), nt, ne)
    for c in (0.0, -0.125, float("nan"), float("inf")):     # a coefficient that is not positive and finite
        t = good.copy()
        t[1, 8] = np.array([c], np.float32).view(np.int32)[0]
        assert statuses(t) == {SHAPE}, c
        with pytest.raises(ValueError, match="coefficient"):
            ops.eqlr.check_table(t, nt, ne)
    for col, val in ((3, 0), (4, 0), (5, 0), (5, 7), (6, 5), (7, 0), (0, -4), (1, -4), (2, -8)):       # K, N, taps, the first units, negative offsets
        assert statuses(edited(1, col, val)) == {SHAPE}, (col, val)
    # a segment that ends behind its buffer: the kernel for every call, the effective weights where the call takes that base
    assert statuses(good, theta_floats=nt - 4) == {SHAPE}
    assert lib.bg_eqlr_check_table(good.ctypes.data, 3, nt, ne - 4) == SHAPE and lib.bg_eqlr_scale_f32(base, nt, base, ne - 4, base, good.ctypes.data, 3, None) == SHAPE
    for args in ((None, nt, base, ne, base), (base, nt, None, ne, base), (base, nt, base, ne, None)):
        assert lib.bg_eqlr_scale_f32(*args, good.ctypes.data, 3, None) == NULL
    for args in ((base + 4, nt, base, ne, base), (base, nt, base + 4, ne, base), (base, nt, base, ne, base + 4)):
        assert lib.bg_eqlr_scale_f32(*args, good.ctypes.data, 3, None) == ALIGN
    assert lib.bg_eqlr_grad_f32(None, nt, base, good.ctypes.data, 3, None) == NULL and lib.bg_eqlr_grad_f32(base, nt, None, good.ctypes.data, 3, None) == NULL
    assert lib.bg_eqlr_grad_f32(base + 4, nt, base, good.ctypes.data, 3, None) == ALIGN and lib.bg_eqlr_grad_f32(base, nt, base + 4, good.ctypes.data, 3, None) == ALIGN
    assert (buf == 7.0).all()


def test_the_store_lays_the_effective_weights_out_in_aligned_segments():
    maker.ensure_library(ROOT)
    m = _wrapped_stack().build("cpu")
    net = m.net()
    table = m.store.eqlr_table(net.eqlr_layers)
    assert table is m.store.eqlr_table(net.eqlr_layers) and table.n == 3
    h = table.host
    assert h[:, 3:6].tolist() == [[27, 8, 9], [100, 8, 25], [256, 2, 1]] and (h[:, :2] % 4 == 0).all()
    assert h[:, 1].tolist() == [0, 432, 2032] and h[:, 2].tolist() == [216, 1232, -1] and m.store.eff.numel() == 2544
    assert h[:, 8].view(np.float32).tolist() == [np.float32(l.coefficient) for l in net.eqlr_layers]
    for l in net.eqlr_layers:
        assert m.store.kernel(l).shape == l.vars["kernel"].shape and m.store.kernel(l).untyped_storage().data_ptr() == m.store.eff.untyped_storage().data_ptr()
        assert (m.store.kernel(l, transposed=True) is None) == (l.kind == "dense")


# ------------------------------------------------------------------ 5. the averaged model's clone
def test_clone_structure_gives_wrappers_and_their_inner_layers_their_own_variables():
    bg.set_seed(4)
    live = models.DCGANGenerator(arch="tiny", equalized_lr=True, normalization="pixel").build("cpu")
    twin = ema.clone_structure(live)
    pairs = [(a, b) for a, b in zip(live._own_layers(), twin._own_layers()) if isinstance(a, EQ)]
    assert len(pairs) == 5
    for a, b in pairs:
        assert isinstance(b, EQ) and b is not a and b.layer is not a.layer and b.coefficient == a.coefficient and b.gain == a.gain
        assert a.layer.vars is a.vars and b.layer.vars is b.vars and b.vars is not a.vars
        for n in a.vars:
            assert torch.equal(a.vars[n], b.vars[n]) and a.vars[n].data_ptr() != b.vars[n].data_ptr() == b.layer.vars[n].data_ptr()
    twin.store.theta.add_(1.0)
    for a, b in pairs:
        assert not torch.equal(a.layer.vars["kernel"], b.layer.vars["kernel"]) and torch.equal(a.vars["kernel"] + 1.0, b.layer.vars["kernel"])
    sn = layers.Sequential([layers.SpectralNormalization(layers.Dense(3, input_shape=(4,)))]).build("cpu")      # the same fix for the other wrapper
    t = ema.clone_structure(sn)
    assert t.layers[0].layer is not sn.layers[0].layer and t.layers[0].layer.vars is t.layers[0].vars and sn.layers[0].layer.vars is sn.layers[0].vars


# ------------------------------------------------------------------ 6. checkpoints
def _gan(critic=True, generator=True, arch="tiny", seed=3, cls=None, **kw):
    cls = cls or bg.WGANGP
    bg.set_seed(seed)
    gen, disc = models.DCGANGenerator(arch=arch, equalized_lr=generator), models.DCGANDiscriminator(arch=arch, equalized_lr=critic)
    gen.build("cpu"), disc.build("cpu")
    return cls(gen, disc, cls.HyperParameters(batch_size=2, global_batch_size=2), bg.TrainingConfig(log_dir=os.devnull), step_replay=False, **kw)


def test_checkpoint_records_the_coefficients_and_refuses_a_model_with_others(tmp_path):
    maker.ensure_library(ROOT)
    a = _gan()
    d = CheckpointManager(a, str(tmp_path)).state_dict()
    assert d["g_eqlr"].dtype == np.float32 and d["g_eqlr"].tolist() == [np.float32(l.coefficient) for l in a.generator.net().eqlr_layers] and len(d["g_eqlr"]) == 5
    assert d["d_eqlr"].tolist() == [np.float32(l.coefficient) for l in a.discriminator.net().eqlr_layers] and len(d["d_eqlr"]) == 3
    path = CheckpointManager(a, str(tmp_path)).save(1)
    b = _gan(seed=8)
    assert not torch.equal(a.generator.store.theta, b.generator.store.theta)
    CheckpointManager(b, str(tmp_path)).restore(path)
    assert torch.equal(a.generator.store.theta, b.generator.store.theta) and torch.equal(a.discriminator.store.theta, b.discriminator.store.theta)
    assert b.generator.store.tr_dirty and b.discriminator.store.tr_dirty
    # a plain model has the same shapes: only the list tells them apart, and the message names both
    for kw, who in ((dict(generator=False), "generator"), (dict(critic=False), "discriminator")):
        plain = _gan(seed=8, **kw)
        before = plain.generator.store.theta.clone()
        with pytest.raises(ValueError, match=who + r".*coefficients \[0\.\d+.*\].*have \[\]"):
            CheckpointManager(plain, str(tmp_path)).restore(path)
        assert torch.equal(before, plain.generator.store.theta)
    plain = _gan(False, False)
    assert CheckpointManager(plain, str(tmp_path)).state_dict()["g_eqlr"].size == 0
    plain_path = CheckpointManager(plain, str(tmp_path / "plain")).save(1)
    with pytest.raises(ValueError, match=r"coefficients \[\].*have \[0\."):
        CheckpointManager(b, str(tmp_path)).restore(plain_path)
    # a file from before the key existed is a plain model's
    old = {k: v for k, v in np.load(plain_path).items() if not k.endswith("_eqlr")}
    old_path = str(tmp_path / "old.npz")
    np.savez(old_path, **old)
    CheckpointManager(_gan(False, False, seed=8), str(tmp_path)).restore(old_path)
    with pytest.raises(ValueError, match=r"coefficients \[\]"):
        CheckpointManager(b, str(tmp_path)).restore(old_path)
    # other gains on the same architecture are another model
    other = _gan(seed=8)
    other.discriminator.net().eqlr_layers[-1].coefficient = _coefficient(SQRT2, 128)
    with pytest.raises(ValueError, match="discriminator"):
        CheckpointManager(other, str(tmp_path)).restore(path)


# ------------------------------------------------------------------ 7. what a step enqueues
EQ_RETURNS = {"scale": "eff", "grad": "grad"}
FORWARDS = ("conv2d_fwd", "conv2d_bwd_data", "gemm", "blur_nhwc", "blur3_lerp", "lerp")


@contextlib.contextmanager
def recording_eqlr(rec):
    with recording(rec):
        saved = {name: ops.eqlr.__dict__[name] for name in EQ_RETURNS}
        for name, ret in EQ_RETURNS.items():
            setattr(ops.eqlr, name, staticmethod(rec.wrap("eqlr." + name, getattr(ops.eqlr, name), ret)))
        try:
            yield rec
        finally:
            for name, old in saved.items():
                setattr(ops.eqlr, name, old)


def _step_events(**kw):
    maker.ensure_library(ROOT)
    rec = _Recorder()
    with recording_eqlr(rec):
        gan = _gan(**kw)
        gan.train_on_batch(np.zeros((2,) + models.IMAGE_SHAPE[kw.get("arch", "tiny")], np.float32))
    return gan, rec.events


def _owner(gan, a):
    G, D = gan.generator.store, gan.discriminator.store
    p = a["theta"].data_ptr() if "theta" in a else a["grad"].data_ptr()
    return "g" if p in (G.theta.data_ptr(), G.grad.data_ptr()) else "d" if p in (D.theta.data_ptr(), D.grad.data_ptr()) else None


@pytest.mark.parametrize("config", [{}, dict(merge_gp_filter_gradients=False), dict(merge_critic_passes=False)])
def test_a_step_of_wrapped_models_enqueues_one_scale_and_one_gradient_launch_per_update(config):
    gan, events = _step_events(**config)
    names = [n for n, _ in events]
    assert "transpose_last2_batched" not in names            # fully wrapped: the scale launch replaces the batched transpose
    adam = [k for k, n in enumerate(names) if n == "adam"]
    assert len(adam) == 2
    eq = [(k, n, _owner(gan, a), a) for k, (n, a) in enumerate(events) if n.startswith("eqlr.")]
    # D-step: both models' weights are new to it; G-step: the critic's changed, the generator's did not
    assert [(n, o) for _, n, o, _ in eq] == [("eqlr.scale", "g"), ("eqlr.scale", "d"), ("eqlr.grad", "d"), ("eqlr.scale", "d"), ("eqlr.grad", "g")]
    assert [a["table"].n for _, _, _, a in eq] == [5, 3, 3, 3, 5]
    first_forward = min(k for k, n in enumerate(names) if n in FORWARDS)
    assert eq[0][0] < first_forward
    finishes = [k for k, n in enumerate(names) if n == "finish"]
    for (k, _, _, _), opt, fin in ((eq[2], adam[0], finishes[0]), (eq[4], adam[1], finishes[1])):
        last_wgrad = max(j for j, n in enumerate(names[:opt]) if n in ("conv2d_bwd_filter", "colsum", "gemm"))
        assert last_wgrad < fin < k == opt - 1                 # behind the all-reduce, directly in front of the optimizer
    assert adam[0] < eq[3][0] < adam[1]
    # the convs and the Dense layers read the effective buffers, never the raw kernels
    inside = lambda t, buf: t.untyped_storage().data_ptr() == buf.untyped_storage().data_ptr()
    effs, thetas = [m.store.eff for m in (gan.generator, gan.discriminator)], [m.store.theta for m in (gan.generator, gan.discriminator)]
    seen = 0
    for n, a in events:
        w = a["wT"] if n == "conv2d_fwd" else a["w"] if n == "conv2d_bwd_data" else a["Bm"] if n == "gemm" and not a["transA"] else None
        if w is not None:
            assert not any(inside(w, t) for t in thetas), n
            seen += any(inside(w, e) for e in effs)
    assert seen >= 8


def test_the_number_of_launches_does_not_depend_on_the_number_of_layers_and_a_half_wrapped_pair_keeps_its_transpose(monkeypatch):
    count = lambda ev: [n for n, _ in ev if n.startswith("eqlr.")]
    base = count(_step_events()[1])
    monkeypatch.setitem(models._D, "tiny", [16, 32, 32])
    gan, ev = _step_events()
    assert len(gan.discriminator.net().eqlr_layers) == 4 and count(ev) == base and len(base) == 5
    monkeypatch.undo()
    gan, ev = _step_events(generator=False)
    assert [(n, _owner(gan, a)) for n, a in ev if n.startswith("eqlr.")] == [("eqlr.scale", "d"), ("eqlr.grad", "d"), ("eqlr.scale", "d")]
    tr = [a for n, a in ev if n == "transpose_last2_batched"]
    assert tr and all(a["src_base"].data_ptr() == gan.generator.store.theta.data_ptr() for a in tr)


def test_plain_models_enqueue_no_eqlr_launch_and_allocate_nothing():
    gan, events = _step_events(critic=False, generator=False)
    assert not [n for n, _ in events if n.startswith("eqlr.")]
    for m in (gan.generator, gan.discriminator):
        assert m.store.eff is None and m.store._eq_table is None and m.net().plain_conv_layers == m.net().conv_layers


def test_generator_ema_is_accepted_with_a_wrapped_generator():
    gan = _gan(generator_ema=0.99)
    E = gan.generator_ema
    assert E is not None and len(E.net().eqlr_layers) == 5 and E.store is not gan.generator.store
    assert all(a is not b and a.layer is not b.layer for a, b in zip(E.net().eqlr_layers, gan.generator.net().eqlr_layers))


# ------------------------------------------------------------------ 8. the code objects
def test_kernels_do_not_spill_and_stream_float4(tmp_path_factory):
    """The reading of tests/test_build_cpu.py::test_hot_kernels_do_not_spill, on csrc/eqlr.hip."""
    import re
    from test_build_cpu import HIPCC, _isa, _resources
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    isa = _isa(tmp_path_factory, "eqlr.hip")
    res = _resources(isa, "_kernel")
    assert len(res) == 2 and all(any(k in n for n in res) for k in ("eqlr_scale", "eqlr_grad")), list(res)
    assert all(v == (0, 0, 0) for v in res.values()), res
    for name in res:            # both have a float4 route, and neither uses an atomic
        body = re.search(r"^" + re.escape(name) + r":(.*?)^\.Lfunc_end", isa, flags=re.S | re.M).group(1)
        assert "global_load_dwordx4" in body and "global_store_dwordx4" in body and "atomic" not in body, name
